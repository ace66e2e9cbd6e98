"""tests/mesh_cull_oracle.py held to facts that do not depend on it: on the mesh of the TSDF tests' integrated volume and the three
frames that made it, the counts a scratch restatement of dqo_mesh_cull's statements gave when the rule was written (per view and
branch, per vertex, per face), the header's identities, the inclusions the rule implies, and — on a fourth view and with `near` — the
"not in front" branch, which the three frames leave empty."""
import numpy as np

import mesh_cull_oracle as C


def _cull(views=slice(0, 3), depth=True, **kw):
    s = C.scene()
    kw.setdefault("eps", C.EPS)
    return C.cull(s["vertices"], s["colors"], s["faces"], s["w2c"][views], s["K"], s["W"], s["H"],
                  depth=s["depth"][views] if depth else None, **kw)


def _count(state, k):
    return [int((state[:, k] == c).sum()) for c in (C.NOT_IN_FRONT, C.OUTSIDE_IMAGE, C.NO_DEPTH, C.OCCLUDED, C.SEEN)]


def test_the_counts_worked_out_with_the_rule():
    s = C.scene()
    V, F = len(s["vertices"]), len(s["faces"])
    assert (V, F) == (6498, 12368)
    r = _cull()
    assert _count(r["state"], 0) == [0, 0, 72, 1098, 5328]
    assert _count(r["state"], 1) == [0, 1590, 0, 1063, 3845]
    assert _count(r["state"], 2) == [0, 3113, 14, 1135, 2236]
    assert np.bincount(r["vertex_views"], minlength=4).tolist() == [253, 1531, 4264, 450]
    assert np.bincount(r["corners"], minlength=4).tolist() == [124, 238, 358, 11648]
    h = r["header"].tolist()
    assert h == [6211, 11648, 6498 - 253, 3, 0, 124 + 238 + 358, 6498 - 6211, 0]
    assert h[2] - h[0] == 34  # seen vertices that no kept face names
    assert r["header"].dtype == np.int32 and r["vertices"].dtype == np.float32 and r["faces"].dtype == np.int32


def _identities(r, V, F, min_corners=3):
    h = r["header"].tolist()
    assert F == h[1] + h[4] + h[5] and V == h[0] + h[6] and h[7] == 0
    assert r["vertices"].shape == (h[0], 3) and r["faces"].shape == (h[1], 3)
    if h[1]:
        assert r["faces"].min() >= 0 and r["faces"].max() < h[0]
    assert len(np.unique(r["faces"])) == h[0]  # every written vertex is named by a kept face
    assert h[2] <= V and (min_corners < 3 or h[0] <= h[2])  # (below three corners a kept face may name a vertex nobody saw)


def test_header_identities_and_inclusions():
    s = C.scene()
    vertices, colors, faces = C.with_extras(s["vertices"], s["colors"], s["faces"])
    V, F = len(vertices), len(faces)
    kept = {}
    for depth in (False, True):
        for mc in (1, 2, 3):
            r = C.cull(vertices, colors, faces, s["w2c"][:3], s["K"], s["W"], s["H"], depth=s["depth"][:3] if depth else None, eps=C.EPS,
                       min_corners=mc)
            _identities(r, V, F, mc)
            assert r["header"][4] == 3  # with_extras' bad faces
            kept[depth, mc] = r["corners"] >= mc
    for depth in (False, True):
        assert (kept[depth, 1] >= kept[depth, 2]).all() and (kept[depth, 2] >= kept[depth, 3]).all()  # min_corners 1 >= 2 >= 3
    assert kept[True, 1].sum() > kept[True, 2].sum() > kept[True, 3].sum()  # (and the inclusions are proper where anything is unseen)
    for mc in (1, 2, 3):
        assert (kept[False, mc] >= kept[True, mc]).all() and kept[False, mc].sum() > kept[True, mc].sum()  # frustum only >= with depth
    # the faces that repeat an index: [0, 0, 5] counts vertex 0 twice
    r = C.cull(vertices, colors, faces, s["w2c"][:3], s["K"], s["W"], s["H"], depth=s["depth"][:3], eps=C.EPS)
    at = len(s["faces"]) // 2
    v = r["vertex_views"]
    assert r["corners"][at] == 2 * int(v[0] > 0) + int(v[5] > 0) and r["corners"][at + 1] == 3 * int(v[3] > 0) and r["corners"][at + 2] == -1


def test_view_keep():
    none = _cull(view_keep=np.zeros(3, np.uint8))
    assert none["header"].tolist() == [0, 0, 0, 0, 0, 12368, 6498, 0] and (none["state"] == C.VIEW_UNUSED).all()
    two, whole = _cull(view_keep=np.array([1, 0, 1], np.uint8)), _cull()
    assert two["header"][3] == 2 and np.array_equal(two["state"][:, [0, 2]], whole["state"][:, [0, 2]])
    only = _cull(views=[0, 2])
    for k in ("vertices", "colors", "faces", "vertex_views"):
        assert two[k].tobytes() == only[k].tobytes(), k


def test_a_mesh_that_is_seen_whole_comes_back_bit_for_bit():
    s = C.scene()
    r = _cull()  # min_corners = 3: every written vertex is a seen corner
    again = C.cull(r["vertices"], r["colors"], r["faces"], s["w2c"][:3], s["K"], s["W"], s["H"], depth=s["depth"][:3], eps=C.EPS)
    assert (again["vertex_views"] > 0).all() and again["header"].tolist() == [6211, 11648, 6211, 3, 0, 0, 0, 0]
    for k in ("vertices", "colors", "faces"):
        assert again[k].tobytes() == r[k].tobytes() and again[k].dtype == r[k].dtype, k


def test_the_not_in_front_branch():
    """The three frames see no vertex behind them; the fourth view and a `near` above some vertices' pc_z do."""
    three = _cull()
    assert not (three["state"] == C.NOT_IN_FRONT).any()
    four = _cull(views=slice(0, 4))
    behind = four["state"][:, 3] == C.NOT_IN_FRONT
    assert 1000 < behind.sum() < 6498 - 1000 and (four["state"][:, 3] == C.SEEN).sum() > 100
    assert np.array_equal(four["state"][:, :3], three["state"])
    s = C.scene()
    z = s["vertices"].astype(np.float64) @ s["w2c"][3].astype(np.float64)[2, :3] + float(s["w2c"][3][2, 3])
    assert (behind == (z <= 0)).all()  # (no vertex within rounding of the camera's plane)
    _identities(four, 6498, 12368)
    near = _cull(near=1.0)
    assert (near["state"] == C.NOT_IN_FRONT).sum() > 1000 and near["header"][1] < three["header"][1]
    # `near` only moves pairs into the branch: whatever it leaves is classified as before
    left = near["state"] != C.NOT_IN_FRONT
    assert np.array_equal(near["state"][left], three["state"][left])
    _identities(near, 6498, 12368)
