"""Mesh evaluation on the GPU (csrc/map_meshcull.hip, map_meshsample.hip): dqo_eval.mesh_cull bit for bit against
tests/mesh_cull_oracle.py — vertices, colours, faces, the eight header words, vertex_views — on the mesh of the TSDF tests' integrated
volume and the frames that made it; dqo_eval.sample_surface_counted byte for byte against sample_surface on the host-sliced mesh;
dqo_eval.eval_mesh and FusedMapper.evaluate_mesh against the chain done by hand; the three operators replayed from a captured graph
with changed counts.  The meshes reach the device as in tests/test_gpu_mesh_ops.py: buffers larger than the counts, NaN positions and
indices of 2^30 behind them.

Bars.  Everything the cull writes: bit for bit (float32 statements without contraction, integer atomics).  The counted sampler: byte
for byte sample_surface's, the same kernels on the same faces.  One sampler case against tests/mesh_oracle.py under the bars of
tests/test_gpu_mesh_sample.py (stated there).  eval_mesh's row against the float64 eval_pcd oracle: the bars of
tests/test_gpu_eval_pcd.py (stated there); their premise — a count is exact when no distance lies at the threshold — is asserted here
at 1e-6 relative, five times the 2e-7 by which a float32 distance differs from scipy's."""
import functools

import numpy as np
import pytest

import mesh_cull_oracle as C
import mesh_oracle as mo
import pcd_oracle as po
import test_gpu_eval_pcd as TP
import test_gpu_mesh_ops as G
import test_gpu_mesh_sample as TS
import test_gpu_tsdf as TT
from test_mesh_oracle import normal_mesh

pytestmark = pytest.mark.gpu

GUARD, GF, GI = 64, 12345.5, -77
THRES = (0.01, 0.03)


def _t(a, dtype=None):
    import torch
    return None if a is None else torch.tensor(np.asarray(a, dtype), device="cuda")


def _upload(vertices, colors, faces, cap_v=None, cap_f=None, counts=None):
    """A mesh dict on the device: capacities above the counts, NaN positions and out-of-range indices behind them, the counts in a
    device header (`counts`: other words than the arrays' lengths)."""
    import torch
    dev = G._dev()
    V, F = len(vertices), len(faces)
    cv, cf = V + G.PAD_V if cap_v is None else cap_v, F + G.PAD_F if cap_f is None else cap_f
    v = torch.full((cv, 3), float("nan"), device=dev)
    f = torch.full((cf, 3), 1 << 30, dtype=torch.int32, device=dev)
    f[F + 1::2] = -7
    v[:V] = torch.from_numpy(np.ascontiguousarray(vertices)).to(dev)
    if F:
        f[:F] = torch.from_numpy(np.ascontiguousarray(faces)).to(dev)
    d = dict(vertices=v, faces=f, header=torch.tensor(list(counts if counts is not None else (V, F)) + [0] * 6, dtype=torch.int32, device=dev))
    if colors is not None:
        d["colors"] = torch.full((cv, 3), float("nan"), device=dev)
        d["colors"][:V] = torch.from_numpy(np.ascontiguousarray(colors)).to(dev)
    return d


def _guarded(cv, cf):
    """An out mesh inside larger buffers, with a vertex_views buffer: (out dict, the four whole buffers)."""
    import torch
    dev = G._dev()
    bv = torch.full((cv * 3 + GUARD,), GF, device=dev)
    bc = torch.full((cv * 3 + GUARD,), GF, device=dev)
    bf = torch.full((cf * 3 + GUARD,), GI, dtype=torch.int32, device=dev)
    bw = torch.full((cv + GUARD,), GI, dtype=torch.int32, device=dev)
    out = dict(vertices=bv[:cv * 3].view(cv, 3), colors=bc[:cv * 3].view(cv, 3), faces=bf[:cf * 3].view(cf, 3), vertex_views=bw[:cv])
    return out, (bv, bc, bf, bw)


def _views(sel):
    """mesh_cull's view arguments for the views `sel` of the scene, on the device."""
    s = C.scene()
    return dict(w2c=_t(s["w2c"][sel].reshape(-1, 16)), K=s["K"], W=s["W"], H=s["H"]), _t(s["depth"][sel])


def _assert_culled(out, want, what, V_in=None):
    import torch
    torch.cuda.synchronize()
    assert out["header"].cpu().numpy().tolist() == want["header"].tolist(), what
    nv, nf = int(want["header"][0]), int(want["header"][1])
    G._same(out["vertices"][:nv], want["vertices"], what + " vertices")
    if want["colors"] is not None:
        G._same(out["colors"][:nv], want["colors"], what + " colors")
    G._same(out["faces"][:nf], want["faces"], what + " faces")
    if out.get("vertex_views") is not None:
        G._same(out["vertex_views"][:V_in], want["vertex_views"], what + " vertex_views")


# ---- the cull against the oracle ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _want(sel, depth, min_corners, keep=None, extras=True, near=0.0):
    s = C.scene()
    v, c, f = C.with_extras(s["vertices"], s["colors"], s["faces"]) if extras else (s["vertices"], s["colors"], s["faces"])
    sel = list(sel)
    return C.cull(v, c, f, s["w2c"][sel], s["K"], s["W"], s["H"], depth=s["depth"][sel] if depth else None,
                  view_keep=None if keep is None else np.array(keep, np.uint8), eps=C.EPS, near=near, min_corners=min_corners)


CULL_CASES = [((0, 1, 2), True, 3, None, 0.0), ((0, 1, 2), True, 2, None, 0.0), ((0, 1, 2), True, 1, None, 0.0), ((0, 1, 2), False, 3, None, 0.0),
              ((0, 1, 2), False, 1, None, 0.0), ((0, 1, 2), True, 3, (1, 0, 1), 0.0), ((0, 1, 2, 3), True, 3, None, 0.0),
              ((0, 1, 2, 3), True, 2, (0, 0, 0, 1), 0.0), ((0, 1, 2), True, 3, None, 1.0)]


@pytest.mark.parametrize("sel, depth, min_corners, keep, near", CULL_CASES)
def test_cull_equals_the_oracle(sel, depth, min_corners, keep, near):
    """With and without vertex_views (the same mesh either way: the early exit must not show), counts below the capacities with the
    rows behind them poisoned, faces with bad and repeated indices among the input's, guard words behind every output, twice."""
    import dqo_eval
    s = C.scene()
    v, c, f = C.with_extras(s["vertices"], s["colors"], s["faces"])
    V, F = len(v), len(f)
    want = _want(sel, depth, min_corners, keep, near=near)
    what = f"views {sel} depth {depth} min_corners {min_corners} keep {keep} near {near}"
    mesh = _upload(v, c, f)
    kw, dep = _views(list(sel))
    kw.update(depth=dep if depth else None, view_keep=_t(keep, np.uint8), eps=float(C.EPS), near=near, min_corners=min_corners)
    cv, cf = V + G.PAD_V, F + G.PAD_F
    out, (bv, bc, bf, bw) = _guarded(cv, cf)
    got = dqo_eval.mesh_cull(mesh, out=out, want_views=True, **kw)
    assert got is out and out["header_names"] == dqo_eval.MESH_CULL_HEADER
    _assert_culled(out, want, what, V)
    nv, nf = int(want["header"][0]), int(want["header"][1])
    assert (bv[3 * nv:] == GF).all() and (bc[3 * nv:] == GF).all() and (bf[3 * nf:] == GI).all() and (bw[V:] == GI).all(), what
    G._tail_untouched(mesh, V, F, what)
    assert mesh["header"].cpu().numpy().tolist()[:2] == [V, F]
    counts = dqo_eval.mesh_counts(out)
    assert tuple(counts) == dqo_eval.MESH_CULL_HEADER and list(counts.values()) == want["header"].tolist()
    # without vertex_views, into the module's own buffers, twice: the same bytes
    for turn in range(2):
        again = dqo_eval.mesh_cull(mesh, **kw)
        assert again is not out and again["vertex_views"] is None and again["vertices"].data_ptr() != out["vertices"].data_ptr()
        _assert_culled(again, want, what + f" no views, turn {turn}")


def test_cull_without_counts_and_without_colours_and_with_the_callers_workspace():
    import torch
    import _dqo_native as N
    import dqo_eval
    s = C.scene()
    V, F = len(s["vertices"]), len(s["faces"])
    mesh = dict(vertices=_t(s["vertices"]), faces=_t(s["faces"]))  # exact buffers, no header: the capacities are the counts
    want = _want((0, 1, 2), True, 3, extras=False)
    assert want["header"].tolist() == [6211, 11648, 6245, 3, 0, 720, 287, 0]  # (tests/test_mesh_cull_oracle.py's counts)
    kw, dep = _views([0, 1, 2])
    need = N.lib().dqo_mesh_cull_workspace_bytes(V, F)
    ws = torch.zeros((need + GUARD,), dtype=torch.uint8, device="cuda")
    ws[need:] = 0xA5
    for turn in range(2):  # the workspace comes back ready for the next call
        out = dqo_eval.mesh_cull(mesh, depth=dep, eps=float(C.EPS), workspace_buffer=ws[:need], want_views=True, **kw)
        assert "colors" not in out
        _assert_culled(out, dict(want, colors=None), f"exact buffers, turn {turn}", V)
        assert (ws[need:] == 0xA5).all()
    # a mesh all of whose vertices are seen comes back bit for bit
    whole = dict(vertices=out["vertices"][:6211].clone(), faces=out["faces"][:11648].clone())
    back = dqo_eval.mesh_cull(whole, depth=dep, eps=float(C.EPS), **kw)
    torch.cuda.synchronize()
    assert back["header"].cpu().numpy().tolist() == [6211, 11648, 6211, 3, 0, 0, 0, 0]
    assert torch.equal(back["vertices"].view(torch.int32), whole["vertices"].view(torch.int32)) and torch.equal(back["faces"], whole["faces"])
    # refusals reach Python as RuntimeError
    own = dict(vertices=torch.empty_like(mesh["vertices"]), faces=torch.empty_like(mesh["faces"]), header=torch.zeros(8, dtype=torch.int32, device="cuda"))
    with pytest.raises(RuntimeError, match="header must not be the input's counts"):
        dqo_eval.mesh_cull(dict(mesh, header=own["header"]), out=own, **kw)
    with pytest.raises(RuntimeError, match="workspace too small"):
        dqo_eval.mesh_cull(mesh, workspace_buffer=ws[:need - 256], **kw)
    with pytest.raises(RuntimeError, match="bad min_corners"):
        dqo_eval.mesh_cull(mesh, min_corners=4, **kw)


def test_cull_smallest_shapes():
    """V = 1 and F = 1; F = 0 through the counts; one view."""
    import dqo_eval
    s = C.scene()
    kw, dep = _views([0])
    for p, seen in (((0.05, -0.02, 1.2), 1), ((0.0, 0.0, -1.0), 0), ((30.0, 0.0, 1.0), 0)):
        v, c, f = np.array([p], np.float32), np.array([[0.25, 0.5, 0.75]], np.float32), np.zeros((1, 3), np.int32)
        want = C.cull(v, c, f, s["w2c"][:1], s["K"], s["W"], s["H"])
        assert want["header"].tolist() == ([1, 1, 1, 1, 0, 0, 0, 0] if seen else [0, 0, 0, 1, 0, 1, 1, 0])
        out = dqo_eval.mesh_cull(_upload(v, c, f, cap_v=1, cap_f=1), want_views=True, **kw)
        _assert_culled(out, want, f"one vertex at {p}", 1)
    v, c, f = C.with_extras(s["vertices"], s["colors"], s["faces"])
    V = len(v)
    want = C.cull(v, c, f[:0], s["w2c"][:1], s["K"], s["W"], s["H"], depth=s["depth"][:1], eps=C.EPS)
    assert want["header"].tolist() == [0, 0, 5328, 1, 0, 0, V, 0]
    out = dqo_eval.mesh_cull(_upload(v, c, f, counts=(V, 0)), depth=dep, eps=float(C.EPS), want_views=True, **kw)
    _assert_culled(out, want, "no faces", V)
    want = C.cull(v[:0], c[:0], f, s["w2c"][:1], s["K"], s["W"], s["H"])  # V = 0 through the counts: every face is bad
    out = dqo_eval.mesh_cull(_upload(v, c, f, counts=(0, len(f))), **kw)
    assert want["header"].tolist() == [0, 0, 0, 1, len(f), 0, 0, 0]
    _assert_culled(out, want, "no vertices")
    # counts above the capacities are clamped
    want = _want((0,), True, 3)
    out = dqo_eval.mesh_cull(_upload(v, c, f, cap_v=V, cap_f=len(f), counts=(1 << 30, 1 << 30)), depth=dep, eps=float(C.EPS), **kw)
    _assert_culled(out, want, "counts above the capacities")


def test_cull_257_views_and_only_the_last_sees_anything():
    """More than one chunk of the 32 views a block walks; views 0 - 255 look away from the mesh."""
    import dqo_eval
    s = C.scene()
    away = s["w2c"][0].copy()
    away[2] = -away[2]
    away[0] = -away[0]  # (a half turn about the y axis: the mesh lies behind)
    w2c = np.concatenate([np.repeat(away[None], 256, 0), s["w2c"][:1]])
    depth = np.concatenate([np.repeat(s["depth"][1:2], 256, 0), s["depth"][:1]])
    v, c, f = C.with_extras(s["vertices"], s["colors"], s["faces"])
    want = _want((0,), True, 3)
    state = C.classify(v, w2c[:2], s["K"], s["W"], s["H"], depth[:2], eps=C.EPS)
    assert (state[:, 0] == C.NOT_IN_FRONT).all() and want["header"][1] > 1000
    kw = dict(w2c=_t(w2c.reshape(-1, 16)), K=s["K"], W=s["W"], H=s["H"], depth=_t(depth), eps=float(C.EPS))
    mesh = _upload(v, c, f)
    for want_views in (True, False):
        out = dqo_eval.mesh_cull(mesh, want_views=want_views, **kw)
        _assert_culled(out, dict(want, header=np.array([*want["header"][:3], 257, *want["header"][4:]], np.int32)), f"257 views {want_views}", len(v))
    keep = np.zeros(257, np.uint8)
    keep[[3, 64, 256]] = 1
    out = dqo_eval.mesh_cull(mesh, want_views=True, view_keep=_t(keep), **kw)
    _assert_culled(out, dict(want, header=np.array([*want["header"][:3], 3, *want["header"][4:]], np.int32)), "257 views, three used", len(v))
    keep[256] = 0
    out = dqo_eval.mesh_cull(mesh, view_keep=_t(keep), **kw)
    import torch
    torch.cuda.synchronize()
    assert out["header"].cpu().numpy().tolist() == [0, 0, 0, 2, 3, len(f) - 3, len(v), 0]


# ---- sample_surface_counted ---------------------------------------------------------------------------------------------------------------
CAP_F = 4096


def _sample_both(v, f, F, count, seed, counts=None):
    """(the counted call on the mesh in a capacity of CAP_F faces with the count word F, sample_surface on the host-sliced mesh, the two
    cumulative tables' first F entries)."""
    import torch
    import dqo_eval
    mesh = _upload(v, None, f[:F], cap_v=len(v) + G.PAD_V, cap_f=CAP_F, counts=counts)
    ws = dqo_eval.mesh_sample_workspace(CAP_F, count, "cuda")
    got = dqo_eval.sample_surface_counted(mesh, count, seed=seed, want_face_index=True, workspace_buffer=ws)
    torch.cuda.synchronize()
    cum = dqo_eval.mesh_cum_view(ws, CAP_F)[:F].cpu().numpy().copy()
    G._tail_untouched(mesh, len(v), F, f"F={F}")
    if F == 0:
        return got, None, cum, None
    ws2 = dqo_eval.mesh_sample_workspace(F, count, "cuda")
    want = dqo_eval.sample_surface(_t(v), _t(f[:F]), count, seed=seed, want_face_index=True, workspace_buffer=ws2)
    torch.cuda.synchronize()
    return got, want, cum, dqo_eval.mesh_cum_view(ws2, F).cpu().numpy().copy()


@pytest.mark.parametrize("F", [0, 1, 1023, 1024, 1025, 2049])
@pytest.mark.parametrize("count", [1, 257, 4099])
def test_sample_counted_equals_sample_surface_on_the_sliced_mesh(F, count):
    assert TS._B() == 1024 and CAP_F == 4 * TS._B()
    v, f = normal_mesh(300, 200, 2049, TS._zero_faces(2049, 1024))
    f = np.roll(f, -2, axis=0)  # (the zero-area faces 0 and 1 go to the end: the slice of one face has area)
    got, want, cum, cum_want = _sample_both(v, f, F, count, seed=F + count)
    if F == 0:  # (sample_surface refuses a mesh without faces; the contract: no area, nothing drawn, nothing searched)
        assert got["header"].cpu().numpy().tolist()[:7] == [0, 0, 0, 0, 61, 0, 0] and not got["keep"].any()
        return
    for k in ("points", "face_index", "keep"):
        assert got[k].dtype == want[k].dtype and got[k].cpu().numpy().tobytes() == want[k].cpu().numpy().tobytes(), (F, count, k)
    assert got["header"][:7].cpu().numpy().tolist() == want["header"][:7].cpu().numpy().tolist()
    assert cum.tobytes() == cum_want.tobytes() and got["header"][0].item() == count and got["keep"].all()  # (something was drawn)


def test_sample_counted_against_the_oracle_clamps_and_an_empty_mesh():
    """One case under the bars of tests/test_gpu_mesh_sample.py (its _check, fed the counted call's outputs); a count word above the
    capacity is clamped; a mesh without area gives no sample."""
    import torch
    import dqo_eval
    F, count, seed = 2049, 4099, 17
    v, f = normal_mesh(300 + F % 97, 200, F, TS._zero_faces(F, 1024))
    mesh = _upload(v, None, f, cap_v=len(v), cap_f=F, counts=(1 << 30, (1 << 31) - 1))  # both words above the capacities
    ws = dqo_eval.mesh_sample_workspace(F, count, "cuda")
    d = dqo_eval.sample_surface_counted(mesh, count, seed=seed, want_face_index=True, workspace_buffer=ws)
    torch.cuda.synchronize()
    got, cum = {k: t.cpu().numpy() for k, t in d.items()}, dqo_eval.mesh_cum_view(ws, F).cpu().numpy().copy()
    o = mo.sample_surface_oracle(v, f, count, seed)
    q_dev, q_or = np.diff(cum, prepend=np.int64(0)), o["q"].astype(np.int64)
    assert (q_dev >= 0).all() and cum[-1] < (1 << 61) and got["header"][4] == o["e"]
    print(f"faces whose quanta differ {int((q_dev != q_or).sum())}")
    assert np.abs(q_dev - q_or).max() <= 1 and ((q_dev == 0) == (q_or == 0)).all()
    dr = mo.draw(v, f, q_dev.astype(np.uint64), count, seed)
    assert dr["total"] == int(cum[-1]) and got["header"].tolist()[:4] == o["header"][:4]
    assert (got["face_index"] == dr["face_index"]).all() and got["points"].view(np.int32).tobytes() == dr["points"].view(np.int32).tobytes()
    assert (got["keep"] == 1).all()
    # no header at all: the capacities; the very points sample_surface yields
    plain = dqo_eval.sample_surface_counted(dict(vertices=_t(v), faces=_t(f)), count, seed=seed)
    ref = dqo_eval.sample_surface(_t(v), _t(f), count, seed=seed)
    torch.cuda.synchronize()
    assert plain["points"].cpu().numpy().tobytes() == got["points"].tobytes() == ref["points"].cpu().numpy().tobytes()
    assert plain["face_index"] is None
    # a mesh without area, and negative count words
    vz, fz = normal_mesh(5, 50, 300, zero=range(300))
    for counts, hdr in (((50, 300), [0, 300, 0, 300, 61 - 9, 0, 0]), ((-5, 300), [0, 300, 300, 0, 61 - 9, 0, 0]), ((50, -1), [0, 0, 0, 0, 61, 0, 0])):
        e = dqo_eval.sample_surface_counted(_upload(vz, None, fz, counts=counts), 257)
        torch.cuda.synchronize()
        assert e["header"][:7].cpu().numpy().tolist() == hdr and not e["keep"].any(), counts


# ---- eval_mesh ----------------------------------------------------------------------------------------------------------------------------
def _rec_of(s):
    """A reconstruction of the scene's mesh: its vertices moved by a smooth centimetre-sized field, its last faces missing."""
    p = s["vertices"].astype(np.float64)
    moved = p + 0.012 * np.stack([np.sin(5 * p[:, 1]), np.cos(4 * p[:, 2]), np.sin(3 * p[:, 0] + 1)], 1)
    return moved.astype(np.float32), s["colors"], s["faces"][:-700]


def _by_hand(rec, gt, n, seed, views):
    """mesh_cull -> read counts -> sample_surface on slices -> eval_pcd; also the two point sets as numpy."""
    import torch
    import dqo_eval
    sets = []
    for m, sd in ((gt, seed), (rec, seed + 1)):
        if views is not None:
            m = dqo_eval.mesh_cull(m, **views)
        c = dqo_eval.mesh_counts(m)
        sets.append(dqo_eval.sample_surface(m["vertices"][:c["vertices"]], m["faces"][:c["faces"]], n, seed=sd))
    row = dqo_eval.eval_pcd(sets[0]["points"], sets[1]["points"], THRES, gt_keep=sets[0]["keep"], rec_keep=sets[1]["keep"])
    torch.cuda.synchronize()
    return row, sets[0]["points"].cpu().numpy(), sets[1]["points"].cpu().numpy()


@pytest.mark.parametrize("culled", [False, True])
def test_eval_mesh_equals_the_chain_by_hand_and_the_oracle(culled):
    import torch
    import dqo_eval
    s = C.scene()
    n, seed = 4099, 21
    rv, rc, rf = _rec_of(s)
    rec, gt = _upload(rv, rc, rf), _upload(s["vertices"], None, s["faces"])
    views = None
    if culled:
        kw, dep = _views([0, 1, 2])
        views = dict(kw, depth=dep, eps=float(C.EPS))
    table = torch.full((3, 32), 7.0, device="cuda")
    got = dqo_eval.eval_mesh(rec, gt, n, seed=seed, dist_thres=THRES, views=views, out=table, row=1)
    hand, gt_pts, rec_pts = _by_hand(rec, gt, n, seed, views)
    assert got.data_ptr() == table[1].data_ptr() and (table[[0, 2]] == 7.0).all()
    assert TP._bits(got).tobytes() == TP._bits(hand).tobytes(), (got.cpu().numpy()[:10], hand.cpu().numpy()[:10])
    # against the float64 oracle, on the oracle's culled meshes (sampled by sample_surface)
    want_m = []
    for v, c, f in ((s["vertices"], None, s["faces"]), (rv, rc, rf)):
        if culled:
            r = C.cull(v, c, f, s["w2c"][:3], s["K"], s["W"], s["H"], depth=s["depth"][:3], eps=C.EPS)
            v, f = r["vertices"], r["faces"]
        want_m.append((v, f))
    pts = [dqo_eval.sample_surface(_t(v), _t(f), n, seed=seed + k)["points"].cpu().numpy() for k, (v, f) in enumerate(want_m)]
    assert pts[0].tobytes() == gt_pts.tobytes() and pts[1].tobytes() == rec_pts.tobytes()
    d_rec, d_gt = po.kdtree_distances(pts[0], pts[1])
    for th in THRES:  # the premise of exact counts
        assert (np.abs(np.concatenate([d_rec, d_gt]) - th) > 1e-6 * th).all(), th
    TP._assert_row(got.cpu().numpy(), n, n, d_rec, d_gt, THRES, f"eval_mesh culled {culled}")
    # without views, a gt mesh without a header yields the very points sample_surface yields (rec_seed chosen by the caller)
    if not culled:
        plain = dqo_eval.eval_mesh(rec, dict(vertices=_t(s["vertices"]), faces=_t(s["faces"])), n, seed=seed, rec_seed=seed + 1, dist_thres=THRES)
        assert TP._bits(plain).tobytes() == TP._bits(hand).tobytes()


def test_eval_mesh_of_a_cull_that_keeps_nothing_is_a_row_of_nan():
    import torch
    import dqo_eval
    s = C.scene()
    rv, rc, rf = _rec_of(s)
    kw, dep = _views([0, 1, 2])
    row = dqo_eval.eval_mesh(_upload(rv, rc, rf), _upload(s["vertices"], None, s["faces"]), 257, dist_thres=THRES,
                             views=dict(kw, depth=dep, view_keep=_t([0, 0, 0], np.uint8)))
    torch.cuda.synchronize()
    assert tuple(row.shape) == (32,) and np.isnan(row.cpu().numpy()).all()
    with pytest.raises(RuntimeError, match="eval_mesh's own"):
        dqo_eval.eval_mesh(_upload(rv, rc, rf), _upload(s["vertices"], None, s["faces"]), 257, views=dict(kw, want_views=True))


# ---- FusedMapper.evaluate_mesh ------------------------------------------------------------------------------------------------------------
def test_evaluate_mesh_equals_eval_mesh_with_the_renders_gathered_by_hand():
    import torch
    import dqo_eval
    from dqo_harness.fused_mapping import FusedMapper
    dev, scene_, cams, settings = TT._map_scene()
    fm = FusedMapper(scene_, settings[0], dev)
    vol = dqo_eval.TsdfVolume(origin=(-1.5, -1.5, 0.2), voxel_length=0.0625, dims=(48, 47, 50), sdf_trunc=0.25, device=dev)
    frames = [None, settings[1], settings[2]]
    mesh = fm.make_mesh(frames, vol, depth_trunc=4.0).extract(400000, 800000)
    counts = dqo_eval.mesh_counts(mesh)
    assert counts["vertices"] > 100 and counts["vertices_dropped"] == 0 and counts["faces_dropped"] == 0
    gv, gf = (_t(a) for a in TS.box_mesh(*TS.BOX))
    n, seed, Wd, Hd = 4099, 5, 160, 120
    kw = dict(sample_nums=n, seed=seed, dist_thres=THRES)
    # mismatched intrinsics: refused before anything is made or launched
    for bad in (settings[1]._replace(tanfovx=1.1 * float(settings[1].tanfovx)), settings[1]._replace(image_width=Wd + 16)):
        with pytest.raises(ValueError, match="another image size or other intrinsics"):
            fm.evaluate_mesh(mesh, gv, gf, frames=[None, bad], depths="render", **kw)
    assert fm._mesh_eval_views == {}
    with pytest.raises(ValueError):
        fm.evaluate_mesh(mesh, gv, gf, frames=None, depths="render", **kw)
    got = fm.evaluate_mesh(mesh, gv, gf, frames=frames, depths="render", eps=0.05, depth_trunc=4.0, **kw).clone()
    # by hand: _maintain_render's own depth for the same cameras
    depth = torch.stack([fm._maintain_render(st).out[1].reshape(Hd, Wd).clone() for st in settings])
    w2c = torch.stack([st.viewmatrix.reshape(4, 4).t().contiguous().reshape(16) for st in settings])
    st = settings[0]
    K = (Wd / (2.0 * float(st.tanfovx)), Hd / (2.0 * float(st.tanfovy)), float(st.cx), float(st.cy))
    views = dict(w2c=w2c, K=K, W=Wd, H=Hd, depth=depth, eps=0.05, depth_trunc=4.0, min_corners=3)
    hand = dqo_eval.eval_mesh(mesh, dict(vertices=gv, faces=gf), n, seed=seed, dist_thres=THRES, views=views).clone()
    torch.cuda.synchronize()
    assert not fm.maintain_overflowed()
    assert TP._bits(got).tobytes() == TP._bits(hand).tobytes()
    assert np.isfinite(got.cpu().numpy()[:3]).all() and got[3].item() == 2  # (distances on both sides; the box is not the map's surface)
    culled = dqo_eval.mesh_counts(dqo_eval.mesh_cull(mesh, **views))
    assert 0 < culled["faces"] <= counts["faces"] and culled["views_used"] == 3
    # the caller's own depth, frustum only, no culling: each takes its path
    own = fm.evaluate_mesh(mesh, gv, gf, frames=frames, depths=depth, eps=0.05, depth_trunc=4.0, **kw).clone()
    frustum = fm.evaluate_mesh(mesh, gv, gf, frames=frames, **kw).clone()
    frustum_hand = dqo_eval.eval_mesh(mesh, dict(vertices=gv, faces=gf), n, seed=seed, dist_thres=THRES, views=dict(views, depth=None, eps=0.03,
                                                                                                                    depth_trunc=float("inf"))).clone()
    table = torch.zeros((2, 32), device=dev)
    whole = fm.evaluate_mesh(mesh, gv, gf, out=table, row=1, **kw)
    whole_hand = dqo_eval.eval_mesh(mesh, dict(vertices=gv, faces=gf), n, seed=seed, dist_thres=THRES).clone()
    torch.cuda.synchronize()
    assert TP._bits(own).tobytes() == TP._bits(hand).tobytes()
    assert TP._bits(frustum).tobytes() == TP._bits(frustum_hand).tobytes()
    assert whole.data_ptr() == table[1].data_ptr() and TP._bits(whole).tobytes() == TP._bits(whole_hand).tobytes() and (table[0] == 0).all()
    # the tensor is what the cull reads: a depth without a measurement sees nothing
    blind = fm.evaluate_mesh(mesh, gv, gf, frames=frames, depths=torch.zeros_like(depth), **kw)
    torch.cuda.synchronize()
    assert np.isnan(blind.cpu().numpy()).all()
    # a sharded mapper is refused for its render only
    shard = FusedMapper(scene_, settings[0], dev, attach_count_reducer=lambda k: k)
    with pytest.raises(NotImplementedError, match="sharded"):
        shard.evaluate_mesh(mesh, gv, gf, frames=frames, depths="render", **kw)
    sharded = shard.evaluate_mesh(mesh, gv, gf, frames=frames, depths=depth, eps=0.05, depth_trunc=4.0, **kw)
    torch.cuda.synchronize()
    assert TP._bits(sharded).tobytes() == TP._bits(hand).tobytes()


# ---- graph capture ------------------------------------------------------------------------------------------------------------------------
def test_one_capture_replayed_with_changed_counts_equals_the_eager_calls():
    import torch
    import dqo_eval
    s = C.scene()
    v, c, f = C.with_extras(s["vertices"], s["colors"], s["faces"])
    V, F = len(v), len(f)
    rv, rc, rf = _rec_of(s)
    rec, gt = _upload(rv, rc, rf), _upload(v, c, f)
    kw, dep = _views([0, 1, 2])
    kw.update(depth=dep, eps=float(C.EPS))
    n = 257

    def chain():
        a = dqo_eval.mesh_cull(gt, want_views=True, **kw)
        ga = dqo_eval.sample_surface_counted(a, n, seed=3, want_face_index=True)
        gb = dqo_eval.sample_surface_counted(rec, n, seed=4)
        row = dqo_eval.eval_pcd(ga["points"], gb["points"], THRES, gt_keep=ga["keep"], rec_keep=gb["keep"])
        return dict(vertices=a["vertices"], faces=a["faces"], header=a["header"], views=a["vertex_views"], points=ga["points"],
                    face_index=ga["face_index"], keep=ga["keep"], sample_header=ga["header"], rec_points=gb["points"], row=row)

    def snapshot(d):
        torch.cuda.synchronize()
        h = d["header"].cpu().numpy()
        kept = d["keep"].bool()  # (a sample that was not drawn has no point: its row keeps whatever the buffer held)
        cut = dict(d, vertices=d["vertices"][:h[0]], faces=d["faces"][:h[1]], views=d["views"][:gt["header"][0].item()],
                   points=d["points"][kept], face_index=d["face_index"][kept])
        return {k: t.cpu().numpy().tobytes() for k, t in cut.items()}

    chain()  # the warm-up: the module's buffers and workspaces exist
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):  # (one stream, no parallel branch)
        out = chain()
    for counts, rcounts in (((V, F), (len(rv), len(rf))), ((V - 900, F // 2), (len(rv), 1025)), ((V, 0), (len(rv), len(rf)))):
        gt["header"][:2] = torch.tensor(counts, dtype=torch.int32, device="cuda")
        rec["header"][:2] = torch.tensor(rcounts, dtype=torch.int32, device="cuda")
        graph.replay()
        got = snapshot(out)
        want = snapshot(chain())
        for k in want:
            assert got[k] == want[k], (counts, k)
        hdr = np.frombuffer(got["header"], np.int32)
        assert hdr[1] + hdr[4] + hdr[5] == counts[1] and hdr[0] + hdr[6] == counts[0]
        if counts[1] == 0:
            assert np.isnan(np.frombuffer(got["row"], np.float32)).all()
        else:
            assert np.isfinite(np.frombuffer(got["row"], np.float32)[:10]).all()
