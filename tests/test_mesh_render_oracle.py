"""tests/mesh_render_oracle.py alone, against analysis: what the rule of dqo_mesh_render_depth (include/dqo_raster.h) promises — exact
depth on a fronto-parallel plane, the diagonal included; no hole inside a welded grid; the unit cube against the analytic ray-box depth;
a result that does not depend on the order of the faces; the lower id on a duplicated face.

Bars.  The cube's hit mask may differ from the analytic one in at most 0.5 % of a view's hit pixels (a pixel centre within rounding of a
silhouette edge); the relative depth error stays at or below 2e-5: float32 corners carry 6e-8 each, the ray-plane quotient amplifies
them by the inverse cosine of the grazing angle, which the seeded views keep below a few hundred."""
import numpy as np

import mesh_render_oracle as R

W, H, K = 64, 48, (55.0, 56.0, 31.5, 23.5)
EYE = np.eye(4, dtype=np.float32)


def test_plane_is_exact_at_every_pixel_and_the_diagonal_belongs_to_someone():
    v = np.array([[-4, -4, 2], [4, -4, 2], [4, 4, 2], [-4, 4, 2]], np.float32)
    f = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    r = R.render(v, f, EYE[None], K, W, H)
    assert (r["depth"].view(np.int32) == np.float32(2.0).view(np.int32)).all()
    assert set(np.unique(r["face_index"])) == {0, 1}
    assert r["header"].tolist() == [1, 0, 2, 0, 0, 2, W * H, 0]
    # a square image with the principal point on the pixel grid: the diagonal's pixel centres lie ON the shared edge, and go to face 0
    sq = R.render(v, f, EYE[None], (20.0, 20.0, 16.0, 16.0), 33, 33)
    assert (sq["depth"] == 2.0).all() and (np.diag(sq["face_index"][0]) == 0).all()
    assert (sq["face_index"][0][np.triu_indices(33, 1)] == 0).all() and (sq["face_index"][0][np.tril_indices(33, -1)] == 1).all()


def test_tilted_welded_grid_has_no_hole():
    v, f = R.grid_mesh(24, 24, (-1.1, -0.9, 2.0), (0.09, 0.004, 0.03), (-0.003, 0.075, 0.02))
    r = R.render(v, f, EYE[None], K, W, H)
    hit = r["depth"][0] > 0
    # the interior: the pixels between a row's first and last hit and between their column's first and last hit
    ys, xs = np.nonzero(hit)
    inside = np.zeros_like(hit)
    for yy in range(ys.min(), ys.max() + 1):
        row = np.nonzero(hit[yy])[0]
        inside[yy, row.min():row.max() + 1] = True
    for xx in range(xs.min(), xs.max() + 1):
        col = np.nonzero(hit[:, xx])[0]
        inside[:, xx] &= (np.arange(H) >= col.min()) & (np.arange(H) <= col.max())
    assert inside.sum() > 1500 and (hit | ~inside).all(), int((inside & ~hit).sum())
    # the grid is a plane: depth against the plane's own
    o, du, dv = np.array([-1.1, -0.9, 2.0]), np.array([0.09, 0.004, 0.03]), np.array([-0.003, 0.075, 0.02])
    n = np.cross(du, dv)
    Y, X = np.meshgrid(np.arange(H, dtype=float), np.arange(W, dtype=float), indexing="ij")
    want = (n @ o) / (n[0] * (X - K[2]) / K[0] + n[1] * (Y - K[3]) / K[1] + n[2])
    rel = np.abs(r["depth"][0][hit] - want[hit]) / want[hit]
    assert rel.max() <= 2e-5, rel.max()


def test_cube_against_the_analytic_ray_box_depth():
    v, f = R.cube_mesh()
    views = R.cube_views(40, seed=11)
    r = R.render(v, f, views, K, W, H)
    assert r["header"][3] == 0 and r["header"][4] == 0 and 6 * 40 <= r["header"][2] <= 12 * 40  # (a face seen edge-on may have no box)
    worst, hits = 0.0, 0
    for k in range(40):
        want = R.ray_box_depth(views[k], K, W, H)
        got = r["depth"][k]
        a, b = want > 0, got > 0
        assert a.sum() > 100
        assert (a != b).sum() <= 0.005 * a.sum(), (k, int((a != b).sum()), int(a.sum()))
        both = a & b
        worst = max(worst, float((np.abs(got[both] - want[both]) / want[both]).max()))
        hits += int(b.sum())
    print(f"cube: {hits} hits, worst relative depth error {worst:.3g}")
    assert worst <= 2e-5, worst
    assert hits == r["header"][6]


def test_shuffled_faces_give_the_same_depth_bit_for_bit():
    s = R.mixed_scene()
    r = R.render(s["vertices"], s["faces"], s["w2c"], s["K"], s["W"], s["H"], near=s["near"])
    perm = np.random.default_rng(5).permutation(len(s["faces"]))
    q = R.render(s["vertices"], s["faces"][perm], s["w2c"], s["K"], s["W"], s["H"], near=s["near"])
    assert r["depth"].tobytes() == q["depth"].tobytes()
    hit = r["face_index"] >= 0
    same = (np.sort(s["faces"][perm][q["face_index"][hit]], 1) == np.sort(s["faces"][r["face_index"][hit]], 1)).all(1)
    assert same.mean() > 0.99  # (the face may differ only where two faces give one depth)
    assert r["header"].tolist()[1:6] == q["header"].tolist()[1:6]
    # the scene does what the GPU test needs of it: every count is alive (degenerate: one pair by a repeated id, one by A == 0)
    h = dict(zip(R.HEADER, r["header"].tolist()))
    assert h["faces_bad_index"] == 3 and h["pairs_near_dropped"] > 0 and h["pairs_degenerate"] == 2 and h["pairs_cooperative"] >= 3
    assert h["pairs_rasterised"] > 1000 and h["pixels_hit"] > 1500


def test_a_duplicated_face_resolves_to_the_lower_id():
    v = np.array([[-1, -1, 2], [1, -1, 2.5], [0, 1, 3]], np.float32)
    f = np.array([[0, 1, 2], [0, 1, 2], [0, 1, 2]], np.int32)
    r = R.render(v, f, EYE[None], K, W, H)
    assert (r["depth"] > 0).sum() > 200 and set(np.unique(r["face_index"])) == {-1, 0}
    r = R.render(v, f[:1], EYE[None], K, W, H, view_keep=[0])
    assert r["header"].tolist() == [0] * 8 and not r["depth"].any() and (r["face_index"] == -1).all()


def test_near_plane_and_truncation():
    v = np.array([[-1, -1, 0.5], [1, -1, 0.5], [0, 1, 3]], np.float32)
    f = np.array([[0, 1, 2]], np.int32)
    assert R.render(v, f, EYE[None], K, W, H, near=1.0)["header"].tolist() == [1, 0, 0, 1, 0, 0, 0, 0]  # crosses: dropped, counted
    assert R.render(v, f, EYE[None], K, W, H, near=3.0)["header"].tolist() == [1, 0, 0, 0, 0, 0, 0, 0]  # behind: silent
    r = R.render(v, f, EYE[None], K, W, H, depth_trunc=1.5)
    assert 0 < (r["depth"] > 0).sum() < (R.render(v, f, EYE[None], K, W, H)["depth"] > 0).sum() and r["depth"].max() <= 1.5
