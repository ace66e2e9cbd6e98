"""GPU: floater pruning (dqo_mapgrowth.prune_cameras / prune_touch / prune_step, FusedMapper.prune_floaters — csrc/map_prune.hip) against
tests/prune_oracle.py.  Every comparison is EXACT: the cameras bit for bit (the kernel and the oracle take the same host cos / sin and
hold adds and multiplies only), every buffer of the state, every byte of a freed row, the counts and the workspace."""
import functools

import numpy as np
import pytest

import lifecycle_cases as lc
import prune_oracle as po

pytestmark = pytest.mark.gpu


# ---- cameras ------------------------------------------------------------------------------------------------------------------------------
def _pose(seed, skew=0.0):
    """(viewmatrix, projection) float32 [4,4] of a random camera; skew > 0: a rotation block that is not orthonormal to float32."""
    from dqo_harness import scenes
    rng = np.random.default_rng(seed)
    R = scenes.rot_yx(float(rng.uniform(-60, 60)), float(rng.uniform(-30, 30)))
    if skew:
        R = R + skew * rng.normal(size=(3, 3))
    cam = scenes.Camera(50, 36, 40.0, 42.0, 24.5, 17.5, R, rng.uniform(-2, 2, 3))
    return cam.world_view_transform.astype(np.float32), cam.projection_matrix.astype(np.float32)


@pytest.mark.parametrize("seed, skew, theta, pixel, zero", [(1, 0.0, 3.0, 17 * 50 + 24, False), (2, 0.0, 3.0, 36 * 50 - 1, False),
                                                            (3, 1e-3, 3.0, 0, False), (4, 0.0, 3.0, 777, True), (5, 0.0, 11.25, 1234, False),
                                                            (6, 5e-2, 0.5, 36 * 50 - 1, True)],
                         ids=["centre", "last_pixel", "skewed_pose", "zero_depth", "other_angle", "skewed_zero_last"])
def test_cameras_equal_the_oracle_bit_for_bit(seed, skew, theta, pixel, zero):
    import torch
    import dqo_mapgrowth as mg
    H, W = 36, 50
    vm, pm = _pose(seed, skew)
    depth = np.random.default_rng(100 + seed).uniform(0.5, 4.0, (H, W)).astype(np.float32)
    if zero:
        depth.reshape(-1)[pixel] = 0.0
    want = po.virtual_cameras(vm, pm, depth, pixel, *po.host_cos_sin(theta))
    assert (want["d"] == -1.0) == zero
    view, proj, focal = mg.prune_cameras(torch.tensor(vm).cuda(), torch.tensor(pm).cuda(), torch.tensor(depth).cuda(), pixel, theta_deg=theta)
    torch.cuda.synchronize()
    assert view.dtype == proj.dtype == focal.dtype == torch.float32 and tuple(view.shape) == tuple(proj.shape) == (4, 4, 4)
    assert torch.equal(view.cpu(), torch.from_numpy(want["viewmatrix"]))
    assert torch.equal(proj.cpu(), torch.from_numpy(want["projmatrix"]))
    assert torch.equal(focal.cpu(), torch.from_numpy(want["focal"]))
    again = mg.prune_cameras(torch.tensor(vm).cuda(), torch.tensor(pm).cuda(), torch.tensor(depth).cuda(), pixel, theta_deg=theta, out=(view, proj, focal))
    assert again[0] is view and again[1] is proj and again[2] is focal
    with pytest.raises(RuntimeError, match="outside"):
        mg.prune_cameras(torch.tensor(vm).cuda(), torch.tensor(pm).cuda(), torch.tensor(depth).cuda(), H * W)


# ---- rows ---------------------------------------------------------------------------------------------------------------------------------
LAYOUTS = dict([("600+200", dict(seed=31)), ("one_row", dict(seed=33, n_alive=1, n_spare=0)), ("all_spare", dict(seed=34, n_alive=0, n_spare=64)),
                ("69000+1100", dict(seed=35, n_alive=69000, n_spare=1100))])
WINDOWS = dict(one_id=(4, 5), empty=(5, 5), all=(-1, 100))


@functools.lru_cache(maxsize=None)
def _row_case(layout, pattern):
    """The shared, read-only inputs of a layout: (state with frame_id, n_touched [4,P] int32, row 0, the last live row): frame ids 1..8 on live rows, 0 on spare rows; camera k
    touches a random eighth of the rows; pattern 0 leaves row 0 and the last live row untouched by all four, pattern 1 has camera 3 alone
    touch both."""
    import torch
    kw = LAYOUTS[layout]
    case = lc.make_case(**kw)
    state = case["state"]
    P = int(state["xyz"].shape[0])
    rng = np.random.default_rng(kw["seed"] + 1000)
    alive = state["alive"].numpy().astype(bool)
    state["frame_id"] = torch.from_numpy(np.where(alive, rng.integers(1, 9, P), 0).astype(np.int32))
    n_touched = (rng.random((4, P)) < 0.125) * rng.integers(1, 50, (4, P))
    live = np.flatnonzero(alive)
    named = [0, int(live[-1])] if live.size else []
    n_touched[:, named] = 0
    if pattern == 1:
        n_touched[3, named] = 7
    return state, torch.from_numpy(n_touched.astype(np.int32)), named, case["kw"]["park"]


def _run_rows(state, n_touched, window, park, overflow_at=None):
    import torch
    import dqo_mapgrowth as mg
    g = {k: v.clone().cuda() for k, v in state.items()}
    P = int(g["xyz"].shape[0])
    ws = mg.prune_workspace(P, "cuda")
    ok = torch.zeros(8, dtype=torch.int32, device="cuda")  # a DqoRastHeader: word 2 is `overflow`
    bad = ok.clone()
    bad[2] = 1
    for k in range(4):
        nt = n_touched[k].cuda()
        if k == overflow_at:
            nt = torch.zeros_like(nt)  # (what an overflowed forward leaves)
        mg.prune_touch(nt, ws, render_header=bad if k == overflow_at else (ok if k % 2 else None))
    stats = mg.prune_step(g, ws, window, park.cuda())
    torch.cuda.synchronize()
    return g, stats, ws


def _assert_state(got, want, what=""):
    import torch
    from dqo_mapgrowth import PRUNE_STATE
    for name, _, _ in PRUNE_STATE:
        g, w = got[name].cpu(), want[name]
        assert g.dtype == w.dtype and torch.equal(g, w), (what, name, (g != w).reshape(g.shape[0], -1).any(1).nonzero().reshape(-1)[:8].tolist())


@pytest.mark.parametrize("window", list(WINDOWS), ids=list(WINDOWS))
@pytest.mark.parametrize("layout", list(LAYOUTS), ids=list(LAYOUTS))
def test_rows_equal_the_oracle(layout, window):
    """The layouts of tests/lifecycle_cases.py (three blocks with a partial last one and scattered spare rows, one row, all spare, 274
    blocks with a ragged last one) under a one-id, an empty and an all-covering window, with row 0 and the last live row untouched
    (pattern 0) or touched by the last camera alone (pattern 1).  Each runs twice: buffers, counts and workspace agree bit for bit and the
    workspace is all zero afterwards."""
    import torch
    from dqo_mapgrowth import PRUNE_STATE
    for pattern in (0, 1):
        state, n_touched, named, park = _row_case(layout, pattern)
        want = po.prune_oracle(state, n_touched.sum(0), WINDOWS[window], park)
        got, stats, ws = _run_rows(state, n_touched, WINDOWS[window], park)
        assert stats.dtype == torch.int32 and stats.tolist() == want["stats"], (pattern, stats.tolist(), want["stats"])
        _assert_state(got, want["state"], pattern)
        assert not bool(ws.any())
        if window == "all" and named:
            fates = {po.FATES[int(want["fate"][r])] for r in named}
            assert fates <= ({"deleted_unstable", "deleted_stable"} if pattern == 0 else {"kept_touched"}), fates
        if window == "empty":
            assert want["stats"][:3] == [0, 0, 0]
        if layout in ("600+200", "69000+1100") and window != "empty":
            assert want["stats"][1] > 0 and want["stats"][2] > 0 and want["stats"][0] > want["stats"][1] + want["stats"][2]
        again, stats2, ws2 = _run_rows(state, n_touched, WINDOWS[window], park)
        assert torch.equal(stats, stats2) and torch.equal(ws, ws2)
        for name, _, _ in PRUNE_STATE:
            assert torch.equal(got[name], again[name]), name


def test_an_overflowed_render_deletes_nothing_and_leaves_the_workspace_clean():
    """Camera 2's header has its overflow word set (and its n_touched is all zero, as an overflowed forward leaves it): nothing is
    deleted, skipped == 1, valid_renders == 3, and the same workspace then serves a valid call that equals the oracle."""
    import torch
    import dqo_mapgrowth as mg
    state, n_touched, named, park = _row_case("600+200", 0)
    want = po.prune_oracle(state, n_touched.sum(0), WINDOWS["all"], park, invalid_renders=1, valid_renders=3)
    assert want["stats"][1] == want["stats"][2] == 0 and want["stats"][3:5] == [3, 1] and want["stats"][0] > 0
    got, stats, ws = _run_rows(state, n_touched, WINDOWS["all"], park, overflow_at=2)
    assert stats.tolist() == want["stats"]
    _assert_state(got, state)  # untouched
    assert not bool(ws.any())
    # the next call on the same buffers and workspace
    for k in range(4):
        mg.prune_touch(n_touched[k].cuda(), ws)
    stats = mg.prune_step(got, ws, WINDOWS["all"], park.cuda(), stats=stats)
    torch.cuda.synchronize()
    want = po.prune_oracle(state, n_touched.sum(0), WINDOWS["all"], park)
    assert stats.tolist() == want["stats"] and want["stats"][1] > 0 and want["stats"][3:5] == [4, 0]
    _assert_state(got, want["state"])
    assert not bool(ws.any())


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def _problem():
    from test_gpu_mapgrowth import _growth_problem
    return _growth_problem(8000)


def _behind_all(cams, n):
    """n points behind all four virtual cameras (p_view.z < 0 for each), beside each other 3 units behind camera 0."""
    V = cams["viewmatrix"].astype(np.float64)  # p_view = p @ V[:3,:3] + V[3,:3]
    c2w = np.linalg.inv(V[0].T)
    p = c2w[:3, 3] - 3.0 * c2w[:3, 2] + 0.05 * np.arange(n)[:, None] * c2w[:3, 0]
    for k in range(4):
        assert ((p @ V[k][:3, 2] + V[k][3, 2]) < -1.0).all()
    return p.astype(np.float32)


def _op_touch_counts(fm, params, view, proj, tile_mask):
    """The four virtual views rendered by the public op on `params`: (sum of n_touched [P] on the host, the fourth render)."""
    import torch
    from dqo_harness import mapping
    total, last = None, None
    for k in range(4):
        last = mapping.render(fm.settings._replace(viewmatrix=view[k].clone(), projmatrix=proj[k].clone()), params, tile_mask=tile_mask)
        nt = last["n_touched"].cpu().long()
        total = nt if total is None else total + nt
    return total, last


def _snapshot(fm):
    from dqo_mapgrowth import PRUNE_STATE
    opacity, scales, rotations = fm.activate()
    params = dict(xyz=fm.xyz.clone(), opacity=opacity.clone(), scales=scales.clone(), rotations=rotations.clone(), shs=fm.shs.clone())
    return {name: getattr(fm, name).clone() for name, _, _ in PRUNE_STATE}, params


def test_prune_floaters_end_to_end_keeps_the_captured_graph():
    """reserve -> track_lifecycle -> capture -> three replays -> prune_floaters on the 8 000-Gaussian growth problem, with a window of
    about 4 000 rows of both clouds, five window rows moved behind the cameras and a tile mask that blanks one band: the oracle gets the
    touch counts the public op returns for the same cameras and parameters.  Afterwards the graph is the same object, not stale, and
    replays; the next grow() stores in place into the freed rows and stamps frame_id; a second call reads nothing back."""
    import torch
    import _dqo_native as N
    from dqo_harness import scenes
    from dqo_harness.fused_mapping import FusedMapper
    from dqo_mapgrowth import PRUNE_STATE
    dev, cam, scene, settings, gt_color, gt_depth, mask = _problem()
    fm = FusedMapper(scene, settings, dev).reserve(1000)
    P, H, W = fm.P, gt_depth.shape[-2], gt_depth.shape[-1]
    assert fm.frame_id is None
    fm.track_lifecycle(stable_mask=torch.arange(P, device=dev) % 2 == 0, tick=0, frame_id=3)
    assert fm.frame_id.dtype == torch.int32 and bool((fm.frame_id[:8000] == 3).all()) and not bool(fm.frame_id[8000:].any())
    fm.frame_id[:8000] = (3 + torch.arange(8000, device=dev) % 4).to(torch.int32)  # ids 3..6; the window (4, 6] holds rows r % 4 in (2, 3)
    window = (4, 6)
    fm.set_training_rows(trainable=~fm.stable_rows())
    fm.begin_mapping_call()
    fm.capture(gt_color, gt_depth, mask)
    for _ in range(3):
        fm.replay()
    graph = fm._g
    projection = torch.tensor(cam.projection_matrix, dtype=torch.float32, device=dev)
    tile_mask = torch.ones(((H + 15) // 16, (W + 15) // 16), dtype=torch.int32, device=dev)
    tile_mask[20:24] = 0
    row, col = po.centre_pixel(cam.cx, cam.cy, H, W)
    assert (row, col) == (int(cam.cx), int(cam.cy))
    want_cams = po.virtual_cameras(fm.settings.viewmatrix.cpu().numpy(), projection.cpu().numpy(), gt_depth.cpu().numpy(), row * W + col,
                                   *po.host_cos_sin(3.0))
    moved = torch.tensor([2, 3, 402, 403, 1002], device=dev)
    fm.xyz[moved] = torch.from_numpy(_behind_all(want_cams, 5)).to(dev)
    before, params = _snapshot(fm)
    park = fm._park_position().cpu()
    stats = fm.prune_floaters(gt_depth, window, projection=projection, tile_mask=tile_mask)
    assert fm._n_spare_stale
    torch.cuda.synchronize()
    assert not fm.prune_overflowed() and not fm.maintain_overflowed()
    view, proj, focal = fm._prune_ctx["cameras"]
    for got, name in ((view, "viewmatrix"), (proj, "projmatrix"), (focal, "focal")):
        assert torch.equal(got.cpu(), torch.from_numpy(want_cams[name])), name
    touched, last = _op_touch_counts(fm, params, view, proj, tile_mask)
    out = fm._maintain_ctx.out
    for k, i in dict(render=0, depth=1, color_index_map=2, depth_index_map=3, n_touched=7).items():
        assert torch.equal(out[i], last[k]), k  # the mapper's own fourth render is the op's
    want = po.prune_oracle({k: v.cpu() for k, v in before.items()}, touched, window, park)
    assert stats.tolist() == want["stats"], (stats.tolist(), want["stats"])
    _assert_state({name: getattr(fm, name) for name, _, _ in PRUNE_STATE}, want["state"])
    fate = want["fate"]
    count = lambda name: int((fate == po.FATES.index(name)).sum())
    assert count("deleted_unstable") > 0 and count("deleted_stable") > 0 and count("kept_touched") > 0, [count(f) for f in po.FATES]
    outside = (fate == po.FATES.index("outside_window")) & (touched == 0)
    assert int(outside.sum()) > 0  # untouched rows outside the window stay
    assert 3000 < want["stats"][0] <= 4000
    assert all(po.FATES[int(fate[r])] in ("deleted_unstable", "deleted_stable") for r in moved.tolist())
    assert torch.equal(fm.shs, params["shs"])
    assert fm._g is graph and not graph.stale and fm.P == P
    fm.replay()
    torch.cuda.synchronize()
    assert not fm.graph_overflowed()
    freed = (want["state"]["alive"] == 0).to(dev) & (before["alive"] != 0)
    assert int(freed.sum().item()) == want["stats"][1] + want["stats"][2]
    for k, v in dict(alive=0, xyz=park.to(dev), opacity_raw=-10.0, scaling_raw=-10.0, row_flags=N.ROW_HIDDEN | N.ROW_FROZEN, confidence=0, stable=0,
                     add_tick=0, depth_error_counter=0, color_error_counter=0, frame_id=0).items():  # (also after a replay: nothing trains them)
        a = getattr(fm, k)[freed]
        assert torch.equal(a, v.to(a.dtype).expand_as(a) if torch.is_tensor(v) else torch.full_like(a, v)), k
    # a second call runs on the context the first one sized: no synchronising call, no device-to-host copy (torch raises on one)
    fm.frame_id[:8000:3] = 9
    before, params = _snapshot(fm)
    park = fm._park_position().cpu()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        stats = fm.prune_floaters(gt_depth, (8, 9), projection=projection, tile_mask=tile_mask)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    touched, _ = _op_touch_counts(fm, params, view, proj, tile_mask)
    want2 = po.prune_oracle({k: v.cpu() for k, v in before.items()}, touched, (8, 9), park)
    assert stats.tolist() == want2["stats"] and want2["stats"][1] > 0 and want2["stats"][2] > 0 and not fm.prune_overflowed()
    _assert_state({name: getattr(fm, name) for name, _, _ in PRUNE_STATE}, want2["state"], "second call")
    assert not bool(fm._prune_ctx["ws"].any())
    # growth stores in place into the freed rows and stamps frame_id
    freed = fm.alive == 0
    freed[8000:] = False
    free_rows = (fm.alive == 0).nonzero().reshape(-1)
    new = {k: np.asarray(v)[:300] for k, v in scenes.surfel_room(86, 3000, n_objects=8).items()}
    st = fm.grow(new, new_mapping_call=True, tick=9, frame_id=12)
    assert st["in_place"] is True and st["added"] > 0 and fm._g is graph and not graph.stale and not fm._n_spare_stale
    assert torch.equal(st["rows"], free_rows[:st["added"]]) and bool(freed[st["rows"]].any())
    assert bool((fm.frame_id[st["rows"]] == 12).all()) and bool((fm.add_tick[st["rows"]] == 9).all())
    new = {k: np.asarray(v)[300:600] for k, v in scenes.surfel_room(86, 3000, n_objects=8).items()}
    st = fm.grow(new, new_mapping_call=True, tick=10)  # frame_id None: the tick
    assert st["in_place"] is True and st["added"] > 0 and bool((fm.frame_id[st["rows"]] == 10).all())


def test_the_frame_id_column_follows_the_other_paths_of_the_mapper():
    """reserve() after track_lifecycle() fills spare rows with 0; the snapshot restores the column; the re-allocating store carries it for
    the kept rows and stamps the new ones; maintain() leaves it to its row; an untracked mapper has no column."""
    import torch
    from dqo_harness import scenes
    from dqo_harness.fused_mapping import FusedMapper
    dev, cam, scene, settings, gt_color, gt_depth, mask = _problem()
    assert FusedMapper(scene, settings, dev).frame_id is None
    fm = FusedMapper(scene, settings, dev).track_lifecycle(tick=5)
    assert bool((fm.frame_id == 5).all()) and fm.frame_id.dtype == torch.int32
    fm.reserve(100)
    assert fm.frame_id.shape[0] == 8100 and not bool(fm.frame_id[8000:].any()) and bool((fm.frame_id[:8000] == 5).all())
    fm.frame_id[:8000] = torch.arange(8000, device=dev, dtype=torch.int32) % 7
    snap = fm._snapshot_state()
    kept = fm.frame_id.clone()
    fm.frame_id.fill_(77)
    fm._restore_state(snap)
    assert torch.equal(fm.frame_id, kept)
    fm.add_tick[1:8000:40] = -500
    fm.maintain(6, gt_color, gt_depth, unstable_time_window=100, stable_confidence_thres=1.0e9, delete_thresh=10 ** 6)
    assert torch.equal(fm.frame_id, kept) and int((fm.alive[:8000] == 0).sum().item()) > 0  # (a freed row keeps a stale frame_id)
    keep = fm.alive.bool().nonzero().reshape(-1)
    new = {k: np.asarray(v)[:300] for k, v in scenes.surfel_room(86, 3000, n_objects=8).items()}
    st = fm.grow(new, new_mapping_call=False, tick=11, frame_id=4)  # (the mapping call goes on: always the re-allocating store)
    nk = keep.numel()
    assert st["in_place"] is False and st["added"] > 0
    assert torch.equal(fm.frame_id[:nk], kept[keep]) and bool((fm.frame_id[nk:nk + st["added"]] == 4).all())
    assert not bool(fm.frame_id[nk + st["added"]:].any())  # the spare rows reserved again


def test_prune_floaters_refuses():
    import torch
    from dqo_harness.fused_mapping import FusedMapper
    dev, cam, scene, settings, gt_color, gt_depth, mask = _problem()
    projection = torch.tensor(cam.projection_matrix, dtype=torch.float32, device=dev)
    fm = FusedMapper(scene, settings, dev)
    with pytest.raises(RuntimeError, match="track_lifecycle"):
        fm.prune_floaters(gt_depth, (0, 1), projection=projection)
    fm = FusedMapper(scene, settings, dev, attach_count_reducer=lambda n: n).track_lifecycle()
    with pytest.raises(NotImplementedError):
        fm.prune_floaters(gt_depth, (0, 1), projection=projection)
    fm = FusedMapper(scene, settings, dev).track_lifecycle()
    before = fm.xyz.clone()
    with pytest.raises(RuntimeError, match="image size"):
        fm.prune_floaters(gt_depth[:, :-1], (0, 1), projection=projection)
    with pytest.raises(RuntimeError, match="image size"):
        fm.prune_floaters(gt_depth, (0, 1), projection=projection, settings=settings._replace(image_height=settings.image_height - 16))
    H = int(settings.image_height)
    with pytest.raises(ValueError, match="outside"):  # the reference's transposed centre: row int(cx)
        fm.prune_floaters(gt_depth, (0, 1), projection=projection, settings=settings._replace(cx=float(H)))
    assert fm._prune_ctx is None and fm._maintain_ctx is None and torch.equal(fm.xyz, before)  # nothing was launched
    stats = fm.prune_floaters(gt_depth, (5, 5), projection=projection, settings=settings._replace(cx=float(H)), centre="principal")
    torch.cuda.synchronize()
    assert stats.tolist()[:3] == [0, 0, 0] and stats.tolist()[3:6] == [4, 0, 8000]
