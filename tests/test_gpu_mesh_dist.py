"""GPU: the nearest face of a mesh per point and the exact point-to-triangle distance (dqo_eval.nearest_on_mesh, dqo_mesh_nearest —
csrc/knn.hip) against tests/mesh_dist_oracle.py.

Bars, and why.  dist2: bit for bit — the kernel and nearest_oracle both return the minimum of one float32 expression, D of
include/dqo_raster.h, over the valid faces; the search's pruning is exact in float (the clamp by the face's box), so the order does not
matter.  face: any valid face whose recomputed D equals dist2 bit for bit.  closest: bit for bit E's x for the RETURNED face.  header:
exactly.  A query that is not searched for, and every query of a mesh without a valid face: FLT_MAX / -1.

Shapes: the face counts around a run of 64 and a box of 1024, one query against 5 000 faces, 70 001 faces (more than 64 boxes: the
group level, a ragged last run), and query counts around a wave and across blocks."""
import numpy as np
import pytest

import mesh_dist_oracle as M
from pcd_oracle import FLT_MAX
from test_mesh_dist_oracle import XFORM, clamp_mesh, fixtures

pytestmark = pytest.mark.gpu


def _t(a, dtype=None):
    import torch
    return None if a is None else torch.tensor(np.asarray(a, dtype), device="cuda")


def _mesh(v, f, counts=None):
    d = dict(vertices=_t(v, np.float32), faces=_t(f, np.int32))
    if counts is not None:
        d["header"] = _t(list(counts) + [0] * 6, np.int32)
    return d


def _check(q, v, f, counts=None, keep=None, xforms=(None, None), what=""):
    """nearest_on_mesh against nearest_oracle under the module's bars.  Returns (dist2, face) as numpy."""
    import torch
    import dqo_eval
    q, v, f = np.asarray(q, np.float32), np.asarray(v, np.float32), np.asarray(f, np.int32)
    d, face, x, h = dqo_eval.nearest_on_mesh(_t(q), _mesh(v, f, counts), _t(keep, np.uint8), xforms[0], xforms[1], want_closest=True)
    torch.cuda.synchronize()
    Q = q.shape[0]
    assert d.dtype == torch.float32 and face.dtype == torch.int32 and tuple(d.shape) == tuple(face.shape) == (Q,) and tuple(x.shape) == (Q, 3)
    d, face, x, h = d.cpu().numpy(), face.cpu().numpy(), x.cpu().numpy(), h.cpu().numpy()
    want_d, want_f, _, want_h = M.nearest_oracle(q, (v, f, counts), keep, xforms)
    wrong = np.nonzero(d.view(np.int32) != want_d.view(np.int32))[0]
    print(f"{what}: Q {Q} F {f.shape[0]} header {h.tolist()} differing dist2 {wrong.size}"
          + (f" first {wrong[0]}: {d[wrong[0]]!r} want {want_d[wrong[0]]!r} face {face[wrong[0]]} want {want_f[wrong[0]]}" if wrong.size else ""))
    assert h.tolist() == want_h.tolist(), what
    assert wrong.size == 0, what
    found = want_f >= 0
    assert ((face >= 0) == found).all() and (face[~found] == -1).all() and (d[~found] == FLT_MAX).all(), what
    valid, _, (a, b, c) = M.face_validity(v, f, counts, xforms[1])
    assert valid[face[found]].all(), what  # (only valid faces are found)
    p = M.transform_f32(q, xforms[0])[found]
    k = face[found]
    D, _, _, xs, _ = M.tri_dist_f32(p, a[k], b[k], c[k])
    assert D.view(np.int32).tobytes() == d[found].view(np.int32).tobytes(), what
    assert xs.view(np.int32).tobytes() == x[found].view(np.int32).tobytes(), what
    return d, face


@pytest.mark.parametrize("name", ["grid", "walls", "slivers", "far"])
def test_the_four_meshes_with_every_kind_of_query(name):
    v, f, q = fixtures()[name]
    d, face = _check(q, v, f, what=name)
    on_surface = d[200:236]  # the queries on vertices, edge midpoints and centroids
    scale = float(np.abs(v).max())
    assert (np.sqrt(on_surface) <= 4 * 2.0 ** -23 * scale).all(), np.sqrt(on_surface).max()


@pytest.mark.parametrize("F", [1, 2, 63, 64, 65, 1023, 1025])
def test_face_counts_around_a_run_and_a_box(F):
    v, f, q = fixtures()["grid"]
    _check(q[:200], v, f[:F], what=f"F {F}")


def test_one_query_against_5000_faces():
    v, f = M.grid_mesh(50, seed=6)
    assert f.shape[0] == 5000
    _check(M.queries(v, f, 1)[:1], v, f, what="Q 1")


def test_70001_faces_use_the_group_level_and_end_in_a_ragged_run():
    v, f = M.grid_mesh(188, seed=7)
    f = f[np.random.default_rng(1).permutation(f.shape[0])[:70001]]
    assert f.shape[0] == 70001 and (70001 + 1023) // 1024 > 64 and 70001 % 64 != 0
    _check(M.queries(v, f, 512 - 40), v, f, what="F 70001")


@pytest.mark.parametrize("Q", [64, 65, 4096])
def test_query_counts_around_a_wave_and_across_blocks(Q):
    v, f, _ = fixtures()["grid"]
    _check(M.queries(v, f[:1025], Q - 40), v, f[:1025], what=f"Q {Q}")


def test_the_nan_fallback_of_a_sliver():
    v, f, q = M.nan_sliver()
    d, face = _check(q, v, f, what="nan sliver")
    assert d[0] == np.float32(26) and face[0] == 0


def test_the_clamp_by_the_faces_box_decides_the_result():
    """tests/mesh_dist_oracle.py's clamp_cases behind the grid's 3200 faces: every query's nearest face is one with B(p, aabb) > E, so
    dist2 must be D — the bits of the minimum of E are others (asserted here) — and the face sits among 50 runs of other faces whose
    records the scan prunes by B."""
    v, f, q, first = clamp_mesh()
    d, face = _check(q, v, f, what="clamp cases")
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    E = M.tri_dist_f32(q[:, None, :], a[None], b[None], c[None])[1]
    differs = d.view(np.int32) != E.min(axis=1).view(np.int32)
    print("clamp cases:", q.shape[0], "dist2 != min E:", int(differs.sum()))
    assert differs.sum() >= 10 and (face >= first).all()
    # the same faces and queries under 70 001 grid faces: more than 64 boxes around them
    gv, gf = M.grid_mesh(188, seed=7)
    cv, cf, cq = M.clamp_cases()
    _check(cq, np.concatenate([gv, cv]), np.concatenate([gf[:70001], cf + gv.shape[0]]), what="clamp cases, 70 001 faces")


def _with_invalid_faces():
    """The grid with every kind of face that is not valid, behind and below the counts: (vertices, faces, counts, rows of the bad faces)."""
    v, f, _ = fixtures()["grid"]
    V, F = v.shape[0], f.shape[0]
    v = np.concatenate([v, np.float32([[0, 0, 5], [1, 0, 5], [2, 0, 5], [np.nan, 0.5, 0.5], [1, 1, 0.1], [1.2, 1, 0.1], [1, 1.2, 0.1]])])
    bad = np.int32([[0, 1, -1], [0, 1, V + 4], [7, 7, 8], [V, V + 1, V + 2], [0, 1, V + 3], [1 << 30, 0, 1]])
    rows = np.arange(0, 60, 10)
    f = np.insert(f, rows, bad, axis=0)  # (among the good faces, so they sit in runs that are scanned)
    behind = np.int32([[V + 4, V + 5, V + 6], [0, 1, 2], [1 << 30, -5, 7]])  # a well-formed face right over (1, 1): never read
    return v, np.concatenate([f, behind]), np.int32([V + 4, F + 6]), rows + np.arange(6)


def test_faces_that_are_not_valid_are_counted_and_never_found():
    v, f, counts, rows = _with_invalid_faces()
    q = np.concatenate([M.queries(v[:-7], f[:-3][np.setdiff1d(np.arange(f.shape[0] - 3), rows)], 300), np.float32([[1.05, 1.05, 0.1], [1, 0, 5]])])
    d, face = _check(q, v, f, counts=counts, what="invalid faces")
    assert not np.isin(face, rows).any() and (face < f.shape[0] - 3).all()
    assert d[-2] > 1e-4  # the face over (1, 1) lies behind the count: the query inside it finds the grid below it


def test_queries_that_are_not_searched_for_and_meshes_without_a_face():
    import torch
    import dqo_eval
    import _dqo_native as N
    v, f, q = fixtures()["grid"]
    keep = np.arange(q.shape[0]) % 3 != 0
    d, face = _check(q, v, f, keep=keep, what="keep")
    assert (face[~keep] == -1).all() and (d[~keep] == FLT_MAX).all()
    _check(q, v, f, keep=np.zeros(q.shape[0], np.uint8), what="nothing kept")
    for counts, what in ((np.int32([v.shape[0], 0]), "no face below the count"), (np.int32([0, f.shape[0]]), "no vertex below the count"),
                         (np.int32([-3, -4]), "negative counts")):
        d, face = _check(q, v, f, counts=counts, what=what)
        assert (face == -1).all() and (d == FLT_MAX).all()
    flat = v.copy()
    flat[:, 1:] = 0  # every face collinear: all below the count, none valid
    d, face = _check(q, flat, f, what="no area")
    assert (face == -1).all()
    # closest rows of queries without a face are not written: the C entry on a buffer of sentinels
    Q = q.shape[0]
    lib = N.lib()
    qd, md, kd = _t(q), _mesh(v, f), _t(keep, np.uint8)
    ws = torch.empty((lib.dqo_mesh_nearest_workspace_bytes(Q, v.shape[0], f.shape[0]),), dtype=torch.uint8, device="cuda")
    d2, fc, hd = torch.empty(Q, device="cuda"), torch.empty(Q, dtype=torch.int32, device="cuda"), torch.empty(8, dtype=torch.int32, device="cuda")
    cl = torch.full((Q, 3), 123.5, device="cuda")
    N.check(lib.dqo_mesh_nearest(Q, qd.data_ptr(), kd.data_ptr(), None, md["vertices"].data_ptr(), md["faces"].data_ptr(), None, v.shape[0],
                                 f.shape[0], None, d2.data_ptr(), fc.data_ptr(), cl.data_ptr(), hd.data_ptr(), ws.data_ptr(), ws.numel(),
                                 N.current_stream()))
    torch.cuda.synchronize()
    cl = cl.cpu().numpy()
    assert (cl[~keep] == 123.5).all() and (cl[keep] != 123.5).any(axis=1).all()


def test_both_transforms_match_the_oracles_restatement():
    v, f, q = fixtures()["grid"]
    full = np.concatenate([XFORM, np.float32([[0, 0, 0, 1]])])
    _check(q, v, f, xforms=(XFORM, None), what="query transform")
    _check(q, v, f, xforms=(None, XFORM), what="mesh transform")
    _check(q, v, f, keep=np.arange(q.shape[0]) % 4 != 1, xforms=(full, full), what="both, [4,4], masked")
    # a mesh stored in another frame comes back under the motion: the distances of the untransformed pair, up to the motion's rounding
    d0, _ = _check(q, v, f, what="plain")
    d1, _ = _check(q, v, f, xforms=(XFORM, XFORM), what="both moved")
    assert np.abs(np.sqrt(d1) - np.sqrt(d0)).max() <= 64 * 2.0 ** -24 * float(np.abs(q).max())


def test_ten_calls_on_one_stream_and_a_captured_graph():
    import torch
    import dqo_eval
    v, f, q = fixtures()["slivers"]
    qd, md = _t(q), _mesh(v, f)
    bits = lambda r: b"".join(t.contiguous().view(torch.int32).cpu().numpy().tobytes() for t in r)
    runs = [dqo_eval.nearest_on_mesh(qd, md, want_closest=True) for _ in range(10)]  # (the module's workspace, shared)
    torch.cuda.synchronize()
    first = bits(runs[0])
    assert all(bits(r) == first for r in runs)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = dqo_eval.nearest_on_mesh(qd, md, want_closest=True)
    for _ in range(2):
        for t in out:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert bits(out) == first


def test_cpu_tensors_raise():
    import torch
    import dqo_eval
    v, f, q = fixtures()["grid"]
    with pytest.raises(RuntimeError, match="no CPU path"):
        dqo_eval.nearest_on_mesh(torch.from_numpy(q), _mesh(v, f))
    with pytest.raises(RuntimeError, match="no CPU path"):
        dqo_eval.nearest_on_mesh(_t(q), dict(vertices=torch.from_numpy(v), faces=torch.from_numpy(f)))
    with pytest.raises(RuntimeError, match="no CPU path"):
        dqo_eval.nearest_on_mesh(_t(q), _mesh(v, f), query_keep=torch.ones(q.shape[0], dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="2\\^25 - 1"):
        dqo_eval.nearest_on_mesh(_t(np.zeros((0, 3), np.float32)), _mesh(v, f))
