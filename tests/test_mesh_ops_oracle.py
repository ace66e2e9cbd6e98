"""tests/mesh_ops_oracle.py held to facts that do not depend on it, on the TSDF oracle's sphere (tsdf_oracle.sphere_volume() -> extract:
3132 vertices, 6260 faces, radius 0.31) and on the archipelago the GPU tests use."""
import numpy as np

import mesh_ops_oracle as M

SPHERE_VOLUME = 4.0 / 3.0 * np.pi * M.SPHERE_R ** 3


def test_the_sphere_is_one_component():
    s = M.sphere()
    assert s["vertices"].shape == (3132, 3) and s["faces"].shape == (6260, 3)
    r = M.components(s["vertices"], s["colors"], s["faces"])
    assert r["header"].tolist() == [3132, 6260, 1, 1, 0, 6260, 0, 0]
    assert (r["labels"] == 0).all()
    assert r["vertices"].tobytes() == s["vertices"].tobytes() and np.array_equal(r["faces"], s["faces"])


def test_a_plain_bfs_gives_the_same_partition_on_the_archipelago():
    a = M.archipelago()
    V = len(a["vertices"])
    labels = M.components(a["vertices"], a["colors"], a["faces"])["labels"]
    assert (labels == -1).sum() == 2
    mine = sorted(sorted(np.nonzero(labels == l)[0].tolist()) for l in np.unique(labels[labels >= 0]))
    assert mine == M.bfs_partition(V, a["faces"])
    assert sorted(len(p) for p in mine) == a["sizes"]
    # a label is the smallest vertex id of its component
    for part in mine:
        assert labels[part[0]] == a["faces"][part].min()


def test_thresholds_on_the_archipelago():
    a = M.archipelago()
    V, F = len(a["vertices"]), len(a["faces"])
    for min_faces, comps, faces in ((0, 9, 6990), (1, 9, 6990), (5, 3, 6969), (8, 3, 6969), (9, 2, 6961), (701, 2, 6961), (6260, 1, 6260),
                                    (6261, 0, 0)):
        h = M.components(a["vertices"], a["colors"], a["faces"], min_faces=min_faces)["header"]
        assert (h[2], h[3], h[1], h[4], h[5]) == (9, comps, faces, 2, 6260), min_faces
        assert h[7] == F - 2 - faces and h[0] + h[6] == V
    r = M.components(a["vertices"], a["colors"], a["faces"], largest_only=True)
    assert r["header"].tolist()[:4] == [3132, 6260, 9, 1] and r["faces"].max() == 3131 and len(np.unique(r["faces"])) == 3132
    # the kept mesh is the sphere up to the renumbering: same positions as a set, same colours with them
    s = M.sphere()
    assert sorted(map(bytes, r["vertices"])) == sorted(map(bytes, s["vertices"]))


def test_every_sphere_vertex_has_4_to_10_neighbours():
    s = M.sphere()
    indptr, idx = M.neighbours(3132, s["faces"])
    deg = np.diff(indptr)
    assert deg.min() >= 4 and deg.max() <= 10 and deg.sum() == 2 * (3132 + 6260 - 2)  # (Euler: E = V + F - 2, each edge twice)
    for i in (0, 1000, 3131):
        n = idx[indptr[i]:indptr[i + 1]]
        assert (np.diff(n) > 0).all() and i not in n
        assert set(n) == set(s["faces"][(s["faces"] == i).any(1)].ravel().tolist()) - {i}


def test_the_centre_of_a_regular_fan_moves_lambda_of_the_way_to_its_rings_centroid():
    """Every ring vertex is as far from the hub as the others, so the weights are equal and S / T is the ring's centroid.  In the ring's
    plane the hub is that centroid already and stays; lifted off the plane it moves lambda of the way."""
    for lift in (0.0, 0.25):
        v, f = M.fan(12, np.array([0.3, -0.2, 0.1]), 0.5, lift=lift)
        for lam in (0.5, 0.25, -0.53):
            p, _ = M.smooth(v.astype(np.float32), None, f, 1, lam=lam)
            want = v[0] + lam * (v[1:].mean(0) - v[0])
            assert np.abs(p[0] - want).max() < 2e-7, (lift, lam)


def _ratios():
    s = M.sphere()
    v0 = M.enclosed_volume(s["vertices"], s["faces"])
    lap, _ = M.smooth(s["vertices"], None, s["faces"], 10, lam=0.5)
    tau, _ = M.smooth(s["vertices"], None, s["faces"], 10, lam=0.5, mu=-0.53)
    return v0 / SPHERE_VOLUME, M.enclosed_volume(lap, s["faces"]) / SPHERE_VOLUME, M.enclosed_volume(tau, s["faces"]) / SPHERE_VOLUME


def test_laplacian_shrinks_and_taubin_keeps_the_volume():
    """Measured with this oracle (volume / the analytic sphere's): unsmoothed 0.9910, ten steps at lambda 0.5: 0.9581, ten Taubin
    iterations (0.5, -0.53): 0.9919."""
    raw, lap, tau = _ratios()
    print(f"volume ratios: unsmoothed {raw:.4f}, laplacian {lap:.4f}, taubin {tau:.4f}")
    assert 0.98 < raw < 1.0
    assert lap < raw - 0.02
    assert abs(tau / raw - 1.0) < 0.01


def test_sphere_normals_are_radial():
    """Measured with this oracle: the smallest normal . radial over the sphere's vertices is 0.9937."""
    s = M.sphere()
    n = M.normals(s["vertices"], s["faces"])
    radial = s["vertices"].astype(np.float64) - M.SPHERE_C
    radial /= np.linalg.norm(radial, axis=1, keepdims=True)
    dots = (n * radial).sum(1)
    print(f"smallest normal . radial: {dots.min():.4f}")
    assert dots.min() > 0.99
    assert np.abs(np.linalg.norm(n.astype(np.float64), axis=1) - 1.0).max() < 1e-6


def test_normals_of_the_extras():
    e = M.smoothing_extras()
    n = M.normals(e["vertices"], e["faces"])
    for i in e["sliver"] + e["isolated"]:
        assert n[i].tolist() == [0.0, 0.0, 1.0]
    indptr, idx = M.neighbours(len(e["vertices"]), e["faces"])
    deg = np.diff(indptr)
    assert deg[e["hubs"][0]] == 300 and deg[e["hubs"][1]] == 2600 and (deg[e["isolated"]] == 0).all()
    raw = np.bincount(e["faces"].ravel(), minlength=len(e["vertices"])) * 2
    assert raw[e["hubs"][0]] == 600 and raw[e["hubs"][1]] == 5200 and 32 < 600 <= 2048 < 5200  # the three paths of the kernels' tidy
