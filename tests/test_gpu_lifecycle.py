"""GPU: map maintenance (dqo_mapgrowth.lifecycle_step, FusedMapper.maintain — csrc/map_lifecycle.hip) against the two-cloud oracle
(tests/lifecycle_oracle.py).  The comparison is EXACT — every integer, flag, tick, clipped confidence and every byte of a freed row — and
each test first asserts that the oracle's float comparisons kept a relative distance of 1e-5 from their thresholds (a smaller one is a
bad fixture, and fails).  Inputs: tests/lifecycle_cases.py."""
import functools

import numpy as np
import pytest

import lifecycle_cases as lc
from lifecycle_oracle import FATES, lifecycle_oracle

pytestmark = pytest.mark.gpu


def _gpu(case):
    import torch
    return {k: v.clone().cuda() for k, v in case["state"].items()}, [case[k].cuda() for k in lc.FRAME], dict(case["kw"], park=case["kw"]["park"].cuda())


def _assert_state(got, want, what=""):
    import torch
    from dqo_mapgrowth import LIFECYCLE_STATE
    for name, _, _ in LIFECYCLE_STATE:
        g, w = got[name].cpu(), want[name]
        assert g.dtype == w.dtype and torch.equal(g, w), (what, name, (g != w).reshape(g.shape[0], -1).any(1).nonzero().reshape(-1)[:8].tolist())


def _oracle(case, state, tick, frame=True, **extra):
    r = lifecycle_oracle(state, tick, *([case[k] for k in lc.FRAME] if frame else [None] * 6), **dict(case["kw"], **extra))
    assert r["margin"] >= 1e-5, r["margin"]
    return r


@pytest.mark.parametrize("kw", [dict(seed=11), dict(seed=12, stable_outlier=True), dict(seed=13, n_alive=1, n_spare=0),
                                dict(seed=14, n_alive=0, n_spare=64), dict(seed=15, n_alive=69000, n_spare=1100, stable_outlier=True)],
                         ids=["600+200", "stable_oversized", "one_row", "all_spare", "69000+1100"])
def test_one_step_equals_the_oracle(kw):
    """Three blocks of 256 with a partial last one, a 50 x 36 frame; index maps that name one row from many pixels, row 0, the last live
    row, -1, spare rows and values outside the map; pixels without a target depth and pixels whose render lies behind the target.  With
    stable_oversized one stable row is 30 x its cloud's mean, which the unstable cloud's mean does not see.  69000+1100 is 274 blocks with
    a ragged last one: 17 ticket lines that 274 is no multiple of, and more partials than the last block folds in one stage, in all three
    row kernels.  Every case runs twice: all buffers, the counts and the workspace agree bit for bit."""
    import torch
    import dqo_mapgrowth as mg
    case = lc.make_case(**kw)
    extra = dict(stable_oversized=True) if kw.get("stable_outlier") else {}
    want = _oracle(case, case["state"], case["tick"], **extra)
    state, frame, th = _gpu(case)
    stats = mg.lifecycle_step(state, case["tick"], *frame, **th, **extra)
    torch.cuda.synchronize()
    assert stats.dtype == torch.int32 and stats.tolist() == want["stats"]
    _assert_state(state, want["state"])
    assert not bool(state["_lifecycle"][1].any())  # every vote word was cleared as it was read
    if "stable_outlier" in case["named"]:
        assert FATES[int(want["fate"][case["named"]["stable_outlier"][0]])] == "deleted_oversized_stable" and want["stats"][5] == 1
    stats = stats.clone()
    again, frame, th = _gpu(case)
    stats2 = mg.lifecycle_step(again, case["tick"], *frame, **th, **extra)
    torch.cuda.synchronize()
    assert torch.equal(stats, stats2) and torch.equal(state["_lifecycle"][2], again["_lifecycle"][2])
    for name, _, _ in mg.LIFECYCLE_STATE:
        assert torch.equal(state[name], again[name]), name


def _run_sequence(case):
    import torch
    import dqo_mapgrowth as mg
    state, frame, th = _gpu(case)
    history = []
    for k in range(lc.SEQUENCE_STEPS):
        stats = mg.lifecycle_step(state, case["tick"] + k, *frame, **th)
        history.append(({n: v.clone() for n, v in state.items() if n != "_lifecycle"}, stats.clone(), state["_lifecycle"][2].clone()))
        bump = lc.sequence_bump(k, case["scripted"])
        if bump:
            state["confidence"].index_fill_(0, torch.tensor(bump[0], device="cuda"), bump[1])
    torch.cuda.synchronize()
    return history


def test_a_sequence_of_twelve_steps_equals_the_oracle_and_repeats_bitwise():
    """delete_thresh = 3 on one state: promotion, three strikes, deletion, release, re-promotion and re-release (tests/lifecycle_cases.py
    scripts them; test_lifecycle_oracle.py checks that they happen).  Compared after every step; run twice: all buffers, the counts and
    the workspace (the two 10 x mean limits among it) agree bit for bit."""
    import torch
    case = lc.sequence_case()
    first, second = _run_sequence(case), _run_sequence(case)
    cpu = case["state"]
    for k in range(lc.SEQUENCE_STEPS):
        want = _oracle(case, cpu, case["tick"] + k)
        assert first[k][1].tolist() == want["stats"], k
        _assert_state(first[k][0], want["state"], k)
        cpu = want["state"]
        bump = lc.sequence_bump(k, case["scripted"])
        if bump:
            cpu["confidence"][bump[0]] = bump[1]
        (rows1, stats1, work1), (rows2, stats2, work2) = first[k], second[k]
        assert torch.equal(stats1, stats2) and torch.equal(work1, work2), k
        for name in rows1:
            assert torch.equal(rows1[name], rows2[name]), (k, name)


def test_without_a_render_counters_and_votes_do_not_move():
    import torch
    import dqo_mapgrowth as mg
    case = lc.make_case(21)
    state, frame, th = _gpu(case)
    mg.lifecycle_step(state, case["tick"], *frame, **th)  # (makes the vote words)
    torch.cuda.synchronize()
    cpu = {k: v.cpu() for k, v in state.items() if k != "_lifecycle"}
    vote = state["_lifecycle"][1]
    vote[::3] = 3  # pending votes a step without a render must neither count nor clear
    pending = vote.clone()
    cpu["confidence"][cpu["alive"].bool() & ~cpu["stable"].bool()] += 15.0
    state["confidence"].copy_(cpu["confidence"])
    want = _oracle(case, cpu, case["tick"] + 1, frame=False)
    assert want["stats"][0] > 0 and want["stats"][1] == want["stats"][2] == 0
    stats = mg.lifecycle_step(state, case["tick"] + 1, *frame[:2], None, None, None, None, **th)
    torch.cuda.synchronize()
    assert stats.tolist() == want["stats"] and torch.equal(vote, pending)
    _assert_state(state, want["state"])
    live = want["state"]["alive"].bool()
    for k in ("depth_error_counter", "color_error_counter"):
        assert torch.equal(state[k].cpu()[live], cpu[k][live])
    with pytest.raises(RuntimeError, match="together or not at all"):
        mg.lifecycle_step(state, 0, *frame[:3], None, None, None, **th)


@functools.lru_cache(maxsize=1)
def _problem():
    from test_gpu_mapgrowth import _growth_problem
    return _growth_problem(8000)


def test_maintain_end_to_end_keeps_the_captured_graph():
    """reserve -> track_lifecycle -> capture -> three replays -> maintain on the 8 000-Gaussian growth problem: the oracle gets the render
    the op returns for the same parameters; afterwards the graph is the same object, not stale, and replays; freed rows are spare rows; the
    next grow() stores in place into them and stamps its rows with its tick."""
    import torch
    import _dqo_native as N
    from dqo_harness import mapping, scenes
    from dqo_harness.fused_mapping import FusedMapper
    from dqo_mapgrowth import LIFECYCLE_STATE
    dev, cam, scene, settings, gt_color, gt_depth, mask = _problem()
    fm = FusedMapper(scene, settings, dev).reserve(1000)
    P, Hh = fm.P, gt_depth.shape[-2]
    assert fm.stable is None
    fm.track_lifecycle(stable_mask=torch.arange(P, device=dev) % 2 == 0, tick=0)
    assert fm.stable.dtype == torch.uint8 and not bool(fm.stable[8000:].any()) and int(fm.stable_rows().sum().item()) == 4000
    fm.set_training_rows(trainable=~fm.stable_rows())
    fm.begin_mapping_call()
    fm.capture(gt_color, gt_depth, mask)
    for _ in range(3):
        fm.replay()
    graph = fm._g
    fm.add_tick[1:8000:50] = -200  # (unstable rows that have been around for too long)
    # a frame that disagrees with the map: the top third lies 0.5 further away, the bottom third is 0.3 brighter
    gt_d = gt_depth.clone()
    gt_d[:, :Hh // 3] += 0.5 * (gt_d[:, :Hh // 3] > 0)
    gt_c = gt_color.clone()
    gt_c[:, 2 * Hh // 3:] += 0.3
    th = dict(stable_confidence_thres=2.0, unstable_time_window=100, add_color_thres=0.1, add_depth_thres=0.1, delete_thresh=1)
    opacity, scales, rotations = fm.activate()
    ref = mapping.render(fm.settings, dict(xyz=fm.xyz, opacity=opacity, scales=scales, rotations=rotations, shs=fm.shs))
    before = {name: getattr(fm, name).clone() for name, _, _ in LIFECYCLE_STATE}
    shs, rot = fm.shs.clone(), fm.rotation_raw.clone()
    stats = fm.maintain(7, gt_c, gt_d, **th)
    assert fm._n_spare_stale
    torch.cuda.synchronize()
    assert not fm.maintain_overflowed()
    out = dict(zip(("render", "depth", "color_index_map", "depth_index_map"), fm._maintain_ctx.out[:4]))
    for k in out:  # maintain's own render is the op's render of the same parameters
        assert torch.equal(out[k], ref[k]), k
    want = lifecycle_oracle({k: v.cpu() for k, v in before.items()}, 7, gt_c.cpu(), gt_d.cpu(), out["render"].cpu(), out["depth"].cpu(),
                            out["depth_index_map"].cpu(), out["color_index_map"].cpu(), park=fm._park_position().cpu(), **th)
    assert want["margin"] >= 1e-5, want["margin"]
    assert stats.tolist() == want["stats"] and all(n > 0 for n in want["stats"][:3]) and want["stats"][4] > 0
    _assert_state({name: getattr(fm, name) for name, _, _ in LIFECYCLE_STATE}, want["state"])
    assert torch.equal(fm.shs, shs) and torch.equal(fm.rotation_raw, rot)
    assert fm._g is graph and not graph.stale and fm.P == P
    fm.replay()
    torch.cuda.synchronize()
    assert not fm.graph_overflowed()
    freed = (want["state"]["alive"] == 0).to(dev) & (before["alive"] != 0)
    assert int(freed.sum().item()) == want["stats"][2] + want["stats"][3] + want["stats"][4]
    park = fm._park_position()
    for k, v in dict(alive=0, xyz=park, opacity_raw=-10.0, scaling_raw=-10.0, row_flags=N.ROW_HIDDEN | N.ROW_FROZEN, confidence=0, stable=0,
                     add_tick=0, depth_error_counter=0, color_error_counter=0).items():  # (also after a replay: nothing trains them)
        a = getattr(fm, k)[freed]
        assert torch.equal(a, v.to(a.dtype).expand_as(a) if torch.is_tensor(v) else torch.full_like(a, v)), k
    # a second call runs on the context the first one sized: no synchronising call, no device-to-host copy (torch raises on one)
    before = {name: getattr(fm, name).clone() for name, _, _ in LIFECYCLE_STATE}
    park = fm._park_position()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        stats = fm.maintain(8, gt_c, gt_d, **th)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    out = [t.cpu() for t in fm._maintain_ctx.out[:4]]
    want2 = lifecycle_oracle({k: v.cpu() for k, v in before.items()}, 8, gt_c.cpu(), gt_d.cpu(), out[0], out[1], out[3], out[2],
                             park=park.cpu(), **th)
    assert want2["margin"] >= 1e-5 and stats.tolist() == want2["stats"] and not fm.maintain_overflowed()
    _assert_state({name: getattr(fm, name) for name, _, _ in LIFECYCLE_STATE}, want2["state"], "second call")
    freed = fm.alive == 0  # (by either call)
    freed[8000:] = False
    free_rows = (fm.alive == 0).nonzero().reshape(-1)
    new = {k: np.asarray(v)[:300] for k, v in scenes.surfel_room(86, 3000, n_objects=8).items()}
    st = fm.grow(new, new_mapping_call=True, tick=9)
    assert st["in_place"] is True and st["added"] > 0 and fm._g is graph and not graph.stale and not fm._n_spare_stale
    assert torch.equal(st["rows"], free_rows[:st["added"]]) and bool(freed[st["rows"]].any())
    assert bool((fm.add_tick[st["rows"]] == 9).all()) and not bool(fm.stable[st["rows"]].any())
    assert not bool(fm.depth_error_counter[st["rows"]].any()) and not bool(fm.color_error_counter[st["rows"]].any())
    assert fm.n_alive + fm._n_spare == fm.P and fm._n_spare == 1000 + int(freed.sum().item()) - st["added"]


def test_an_untracked_or_sharded_mapper_refuses():
    from dqo_harness.fused_mapping import FusedMapper
    dev, cam, scene, settings, gt_color, gt_depth, mask = _problem()
    fm = FusedMapper(scene, settings, dev)
    assert fm.stable is None and fm.add_tick is None and fm.depth_error_counter is None and fm.color_error_counter is None
    with pytest.raises(RuntimeError, match="track_lifecycle"):
        fm.maintain(0, gt_color, gt_depth)
    with pytest.raises(RuntimeError, match="track_lifecycle"):
        fm.stable_rows()
    fm = FusedMapper(scene, settings, dev, attach_count_reducer=lambda n: n).track_lifecycle()
    with pytest.raises(NotImplementedError):
        fm.maintain(0, gt_color, gt_depth)


def test_lifecycle_buffers_follow_the_other_paths_of_the_mapper():
    """maintain() on a mapper that never reserve()d makes `alive`; grow(tick=...) through the re-allocating store carries the four buffers
    of the kept rows and stamps the new ones; the state snapshot restores them."""
    import torch
    from dqo_harness import scenes
    from dqo_harness.fused_mapping import FusedMapper
    dev, cam, scene, settings, gt_color, gt_depth, mask = _problem()
    fm = FusedMapper(scene, settings, dev).track_lifecycle(stable_mask=torch.arange(8000, device=dev) % 3 == 0, tick=5)
    assert fm.alive is None
    fm.add_tick[1:8000:40] = -500
    gone = torch.zeros(8000, dtype=torch.bool, device=dev)
    gone[1:8000:40] = True
    gone &= ~fm.stable_rows()
    stats = fm.maintain(6, gt_color, gt_depth, unstable_time_window=100, stable_confidence_thres=1.0e9, delete_thresh=10 ** 6)
    torch.cuda.synchronize()
    s = stats.tolist()
    dead = fm.alive == 0
    assert fm.alive is not None and fm.P == 8000 and bool(dead[gone].all()) and int(gone.sum().item()) > 0
    assert s[:3] == [0, 0, 0] and s[5] == 0 and s[3] + s[4] == int(dead.sum().item()) and s[4] >= int(gone.sum().item()) - s[3]
    assert s[6] == int((~fm.stable_rows() & ~dead).sum().item()) and s[7] == int(fm.stable_rows().sum().item()) == 2667
    assert not bool(dead[fm.stable_rows()].any())
    # the snapshot carries the four buffers
    snap = fm._snapshot_state()
    kept = {k: getattr(fm, k).clone() for k in ("stable", "add_tick", "depth_error_counter", "color_error_counter")}
    fm.stable.fill_(1), fm.add_tick.fill_(77), fm.depth_error_counter.fill_(3), fm.color_error_counter.fill_(4)
    fm._restore_state(snap)
    for k, v in kept.items():
        assert torch.equal(getattr(fm, k), v), k
    # the re-allocating store: no spare rows were reserved, so the rows maintain() freed leave with the compaction
    fm.depth_error_counter[0:8000:7] = 2
    old = {k: getattr(fm, k).clone() for k in kept}
    new = {k: np.asarray(v)[:300] for k, v in scenes.surfel_room(86, 3000, n_objects=8).items()}
    st = fm.grow(new, new_mapping_call=False, tick=11)  # (the mapping call goes on: always the re-allocating store)
    keep = (~dead).nonzero().reshape(-1)
    nk = keep.numel()
    assert st["in_place"] is False and st["added"] > 0 and fm.P == nk + st["added"] and fm.alive is None
    for k, v in old.items():
        assert torch.equal(getattr(fm, k)[:nk], v[keep]), k
    rows = slice(nk, nk + st["added"])
    assert bool((fm.add_tick[rows] == 11).all()) and not bool(fm.stable[rows].any())
    assert not bool(fm.depth_error_counter[rows].any()) and not bool(fm.color_error_counter[rows].any())
