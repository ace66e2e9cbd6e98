"""GPU: the keyframe bank (csrc/map_window_bank.hip; FusedMapper.capture_bank / run_bank / bank_set / refresh_bank).  The select launch
alone against its numpy restatement (tests/window_bank_oracle.py), byte for byte, and ONE captured graph training over a keyframe set
against the per-frame path (capture_window + run_window, set_frame's graphs), bit for bit: no tolerance anywhere."""
import ctypes
import random

import numpy as np
import pytest

from dqo_harness import scenes
import window_bank_oracle as O

pytestmark = pytest.mark.gpu

P_TRAIN = 12000


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available()
    import _dqo_native as N
    N.lib()
    return torch, N


# ---------------------------------------------------------------------------------------------------- 1. select alone ---------------
PAD = 64  # sentinel bytes on both sides of a destination
SENTINEL, POISON = 0xA5, 0x5C
SCHEDULE = [(0, 0), (0, 0), (1, 0), (1, 2), (2, 2), (2, 2)]
DST_OF = dict(bg="dst_bg", viewmatrix="dst_viewmatrix", projmatrix="dst_projmatrix", campos="dst_campos", gt_color="dst_gt_color",
              gt_depth="dst_gt_depth", render_mask="dst_render_mask", tile_mask="dst_tile_mask", pixel_object="dst_pixel_object",
              tile_objects="dst_tile_objects")
CAMERA_NAMES = tuple(n for n, _, _ in O.CAMERA) + O.CAMERA_GROUP


class _Destination:
    """One slot's worth of every part, each inside a larger byte buffer with sentinels on both sides; the render mask starts W % 4 bytes
    further in, so an odd width also leaves the destination's alignment."""

    def __init__(self, torch, expect, W):
        self.torch, self.buf, self.lead = torch, {}, {}
        for name, a in expect.items():
            lead = PAD + (W % 4 if name == "render_mask" else 0)
            self.lead[name] = lead
            self.buf[name] = torch.full((lead + a.nbytes + PAD,), SENTINEL, dtype=torch.uint8, device="cuda")
            self.write(name, a)

    def ptr(self, name):
        return self.buf[name].data_ptr() + self.lead[name]

    def write(self, name, a):
        raw = np.frombuffer(np.ascontiguousarray(a).tobytes(), np.uint8).copy()
        self.buf[name][self.lead[name]:self.lead[name] + raw.size] = self.torch.from_numpy(raw).cuda()

    def check(self, expect, what):
        for name, a in expect.items():
            got = self.buf[name].cpu().numpy()
            lead, n = self.lead[name], a.nbytes
            assert np.array_equal(got[lead:lead + n], np.frombuffer(np.ascontiguousarray(a).tobytes(), np.uint8)), (what, name)
            assert (got[:lead] == SENTINEL).all() and (got[lead + n:] == SENTINEL).all(), (what, name, "sentinel")


def _poison(a):
    a.view(np.uint8)[...] = POISON


def _select_problem(env, W, H, gate, n_list=8):
    torch, N = env
    rng = np.random.default_rng(W * 131 + H + (7 if gate else 0))
    bank = O.make_bank(rng, 3, W, H, gate)
    dev_bank = {k: torch.from_numpy(v).cuda() for k, v in bank.items() if v is not None}
    expect = O.make_destination(bank)
    dst = _Destination(torch, expect, W)
    i32 = dict(dtype=torch.int32, device="cuda")
    sched = torch.zeros((n_list, 2), **i32)
    lost = torch.full((n_list,), -7, **i32)
    state = torch.full((N.WINDOW_BANK_STATE_WORDS,), 0x55, **i32)  # (arm writes all of it)
    header = torch.zeros((8,), **i32)
    args = N.DqoWindowBank(W=W, H=H, K_cap=3, n=n_list, schedule=sched.data_ptr(), state=state.data_ptr(), lost=lost.data_ptr(),
                           render_header=header.data_ptr(), **{k: v.data_ptr() for k, v in dev_bank.items()},
                           **{DST_OF[k]: dst.ptr(k) for k in expect})
    keep = (dev_bank, sched, lost, state, header)
    return bank, expect, dst, args, keep


def _words(N, state):
    return state[N.TICKET_WORDS:N.TICKET_WORDS + len(O.WORDS)].cpu().numpy()


def _arm(env, keep, schedule):
    torch, N = env
    _, sched, _, state, _ = keep
    sched[:len(schedule)] = torch.tensor(schedule, dtype=torch.int32, device="cuda").reshape(-1, 2)
    N.check(N.lib().dqo_window_bank_arm(state.data_ptr(), len(schedule), N.current_stream()))
    torch.cuda.synchronize()
    assert int(state[:N.TICKET_WORDS].abs().max()) == 0 and int(state[N.TICKET_WORDS + len(O.WORDS):].abs().max()) == 0
    return O.arm(len(schedule))


@pytest.mark.parametrize("gate", [False, True])
@pytest.mark.parametrize("W,H", [(33, 17), (16, 16), (64, 48)])
def test_select_against_the_oracle(env, W, H, gate):
    torch, N = env
    lib = N.lib()
    bank, expect, dst, args, keep = _select_problem(env, W, H, gate)
    _, sched, lost, state, header = keep
    ostate = _arm(env, keep, SCHEDULE)
    assert np.array_equal(_words(N, state), O.state_words(ostate))
    olost = np.full(lost.shape[0], -7, np.int32)
    overflow_before = [1, 1, 0, 1, 1, 0]  # the header's overflow word when launch i runs (launch 0 has no frame behind it)
    groups = dict(camera=[n for n in CAMERA_NAMES if n in expect], masks=list(O.MASK_GROUP))
    for i, (k, m) in enumerate(SCHEDULE):
        if i == 5:  # a repeated entry under force: both groups are copied again
            state[N.TICKET_WORDS + O.WORDS.index("force")] = 1
            ostate["force"] = 1
        changes = dict(camera=ostate["force"] != 0 or k != ostate["prev_k"], masks=ostate["force"] != 0 or m != ostate["prev_m"])
        assert (i, changes) in [(0, dict(camera=True, masks=True)), (1, dict(camera=False, masks=False)), (2, dict(camera=True, masks=False)),
                                (3, dict(camera=False, masks=True)), (4, dict(camera=True, masks=False)), (5, dict(camera=True, masks=True))]
        poisoned = [n for g, names in groups.items() for n in names if not changes[g] or i == 5]
        for n in poisoned:  # a group that does not change keeps the poison: the skip; under force the poison is overwritten
            _poison(expect[n])
            dst.write(n, expect[n])
        header[2] = overflow_before[i]
        wrote = O.select(ostate, bank, expect, SCHEDULE, olost, overflow=bool(overflow_before[i]), list_entries=lost.shape[0])
        assert set(wrote) == {n for g, names in groups.items() for n in names if changes[g]}
        N.check(lib.dqo_window_bank_select(ctypes.byref(args), N.current_stream()))
        torch.cuda.synchronize()
        dst.check(expect, f"launch {i}")
        assert np.array_equal(_words(N, state), O.state_words(ostate)), i
        assert int(state[:N.TICKET_WORDS].abs().max()) == 0  # the ticket is handed back at zero
    assert ostate["lost_count"] == 3 and np.array_equal(lost.cpu().numpy(), olost) and olost[:3].tolist() == [0, 2, 3]
    # a seventh launch: nothing is copied, overrun is set, the cursor stays
    for n in expect:
        _poison(expect[n])
        dst.write(n, expect[n])
    header[2] = 1
    assert O.select(ostate, bank, expect, SCHEDULE, olost, overflow=True, list_entries=lost.shape[0]) == []
    N.check(lib.dqo_window_bank_select(ctypes.byref(args), N.current_stream()))
    torch.cuda.synchronize()
    dst.check(expect, "overrun")
    assert ostate["overrun"] == 1 and ostate["cursor"] == 6 and np.array_equal(_words(N, state), O.state_words(ostate))
    assert np.array_equal(lost.cpu().numpy(), olost)
    # an entry that names no slot: nothing is copied, overrun = 2
    bad = [(1, 1), (3, 0)]
    ostate = _arm(env, keep, bad)
    for i in range(2):
        O.select(ostate, bank, expect, bad, olost, list_entries=lost.shape[0])
        N.check(lib.dqo_window_bank_select(ctypes.byref(args), N.current_stream()))
        torch.cuda.synchronize()
        dst.check(expect, f"bad index {i}")
        assert np.array_equal(_words(N, state), O.state_words(ostate)), i
    assert ostate["overrun"] == 2 and ostate["cursor"] == 1


@pytest.mark.parametrize("W,H,gate", [(33, 17, True), (64, 48, False)])
def test_select_in_a_captured_graph_gives_the_same_sequence(env, W, H, gate):
    torch, N = env
    bank, expect, dst, args, keep = _select_problem(env, W, H, gate)
    _, sched, lost, state, header = keep
    _arm(env, keep, SCHEDULE)
    N.check(N.lib().dqo_window_bank_select(ctypes.byref(args), N.current_stream()))  # (the kernel is loaded before the capture)
    ostate = _arm(env, keep, SCHEDULE)
    olost = np.full(lost.shape[0], -7, np.int32)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        N.check(N.lib().dqo_window_bank_select(ctypes.byref(args), N.current_stream()))
    for i in range(len(SCHEDULE)):
        O.select(ostate, bank, expect, SCHEDULE, olost, list_entries=lost.shape[0])
        graph.replay()
        torch.cuda.synchronize()
        dst.check(expect, f"replay {i}")
        assert np.array_equal(_words(N, state), O.state_words(ostate)), i
    assert ostate["cursor"] == 6 and ostate["lost_count"] == 0


# ---------------------------------------------------------------------------------------------------- 2 - 8. training ----------------
def _cameras(n):
    return [scenes.replica_camera(yaw=12.0 + 3.5 * k, pitch=4.0 - 1.5 * k, pos=(0.3 + 0.15 * k, 0.1 - 0.03 * k, -1.85 + 0.12 * k)) for k in range(n)]


_PROBLEMS = {}


def _window_problem(torch, n_frames, seed=0, gate=False):
    """tests/test_gpu_window.py's recipe at P = 12000 (computed once per (n_frames, seed, gate) and left unchanged: _frames_of copies)."""
    key = (n_frames, seed, gate)
    if key not in _PROBLEMS:
        from dqo_harness import mapping
        _, sc = scenes.make_config(3, P=P_TRAIN)
        dev = torch.device("cuda")
        frames = []
        for k, cam in enumerate(_cameras(n_frames)):
            st = mapping.make_settings(cam, dev)
            tgt = mapping.perturbed_target(sc, st, dev, 100 + 7 * k + seed)
            rng = np.random.default_rng(50 + k)
            mask = torch.tensor(rng.uniform(size=(cam.H, cam.W)) < 0.8, device=dev) & (tgt["pix_obj"] >= 0)
            fr = dict(settings=st, gt_color=tgt["gt_color"].contiguous(), gt_depth=tgt["gt_depth"].contiguous(),
                      render_mask=mask.to(torch.uint8).contiguous())
            if gate:
                fr["pixel_object"] = tgt["pix_obj"].contiguous()
            frames.append(fr)
        _PROBLEMS[key] = (sc, frames, dev)
    return _PROBLEMS[key]


def _frames_of(frames, own_tile_mask=False):
    """Copies a mapper may write in place (capture_window reads the tensors it is given; refresh_window writes them)."""
    import torch
    out = []
    for fr in frames:
        c = {k: (v if k == "settings" else v.clone()) for k, v in fr.items()}
        if own_tile_mask:
            H, W = fr["render_mask"].shape
            c["tile_mask"] = torch.ones(((H + 15) // 16, (W + 15) // 16), dtype=torch.int32, device=fr["render_mask"].device)
        out.append(c)
    return out


def _mapper(torch, sc, frames, dev, gate=False):
    from dqo_harness.fused_mapping import FusedMapper
    fm = FusedMapper(sc, frames[0]["settings"], dev)
    if gate:
        fm.set_object_gate(np.asarray(sc["obj_id"], np.int32), frames[0]["pixel_object"])
    fm.begin_mapping_call(reset_optimizer=True)
    return fm


def _assert_same_training(torch, a, ga, b, gb):
    """Every parameter, both moments of every group, confidence, loss, the step counts and the nine outputs of the last iteration."""
    torch.cuda.synchronize()
    for k in a._params():
        assert torch.equal(a._params()[k], b._params()[k]), k
        assert torch.equal(a.state[k][0], b.state[k][0]) and torch.equal(a.state[k][1], b.state[k][1]), k
    assert torch.equal(a.confidence, b.confidence) and torch.equal(a.loss, b.loss)
    assert a.step_count == b.step_count and int(a._step_dev.item()) == int(b._step_dev.item()) == a.step_count + 1
    for i, (x, y) in enumerate(zip(ga.out, gb.out)):
        assert torch.equal(x, y), i


def _bank_against_window(env, sched, n_frames=3, seed=0, gate=False, **bank_kw):
    torch, _ = env
    sc, frames, dev = _window_problem(torch, n_frames, seed, gate)
    a, b = _mapper(torch, sc, frames, dev, gate), _mapper(torch, sc, frames, dev, gate)
    before = [p.clone() for p in a._params().values()]
    a.capture_bank(_frames_of(frames), loss_tap=True, fused_tail=True, **bank_kw)
    assert a.step_count == 0 and all(torch.equal(x, y) for x, y in zip(before, a._params().values()))  # the capture's iteration is undone
    b.capture_window(_frames_of(frames), loss_tap=True, fused_tail=True)
    assert a.run_bank(sched) == [] and b.run_window(sched) == 0
    assert a.step_count == len(sched)
    _assert_same_training(torch, a, a._bank.graph, b, b._g)
    return a, b


def test_local_loop_on_one_graph_equals_the_per_frame_graphs(env):
    from dqo_harness.fused_mapping import FusedMapper
    sched = FusedMapper.window_schedule(12, 3, random.Random(2))
    assert len(set(sched[:6])) > 1 and sched[7:] == [2] * 5, sched
    a, _ = _bank_against_window(env, sched)
    assert len(a._frames) == 0 and a._bank.graph is not None and float(a.confidence.max()) >= 4


def test_global_loop_with_mixed_pairs_equals_the_mixed_graphs(env):
    from dqo_harness.fused_mapping import FusedMapper
    sched = FusedMapper.window_schedule(12, 3, random.Random(3), global_opt=True)
    assert any(isinstance(e, tuple) for e in sched[7:]) and not any(isinstance(e, tuple) for e in sched[:7]), sched
    _bank_against_window(env, sched, seed=3)


def test_four_iterations_per_launch_are_the_single_launches_bit_for_bit(env):
    torch, _ = env
    from dqo_harness.fused_mapping import FusedMapper
    sched = FusedMapper.window_schedule(11, 3, random.Random(4), final=True)
    assert len(set(sched[:4])) > 1 and len(set(sched[4:8])) > 1, sched  # the frame changes inside a launch of four
    sc, frames, dev = _window_problem(torch, 3, 7)
    ms = []
    for unroll in (1, 4):
        fm = _mapper(torch, sc, frames, dev)
        fm.capture_bank(_frames_of(frames), loss_tap=True, fused_tail=True, unroll=unroll)
        assert (fm._bank.graph.run_graph is not None) == (unroll > 1)
        assert fm.run_bank(sched, check_every=8) == []
        ms.append(fm)
    _assert_same_training(torch, ms[0], ms[0]._bank.graph, ms[1], ms[1]._bank.graph)


def test_run_bank_retries_exactly_the_lost_positions(env):
    torch, _ = env
    sc, frames, dev = _window_problem(torch, 3, 5)
    sched = [0, 1, 2, 1, 1, 0, 2, 1, 0, 2]
    a = _mapper(torch, sc, frames, dev)
    a.capture_bank(_frames_of(frames), loss_tap=True, fused_tail=True, capacity_margin=0.05)  # room for 5 % of the candidate pairs
    tight = a._bank.graph
    retried = a.run_bank(sched, check_every=4)
    torch.cuda.synchronize()
    assert retried and len(set(retried)) == len(retried) and a._bank.graph is not tight
    assert a.step_count == len(sched) and int(a._step_dev.item()) == len(sched) + 1
    order = [p for p in range(len(sched)) if p not in retried] + retried  # what the mapper trained, in the order it trained it
    b = _mapper(torch, sc, frames, dev)
    b.capture_bank(_frames_of(frames), loss_tap=True, fused_tail=True, capacity_margin=2.0)
    assert b.run_bank([sched[p] for p in order]) == []
    _assert_same_training(torch, a, a._bank.graph, b, b._bank.graph)


def test_bank_set_fills_a_spare_slot_without_a_new_capture(env):
    torch, _ = env
    from dqo_harness.fused_mapping import FusedMapper
    sc, frames, dev = _window_problem(torch, 3, 6)
    sched = FusedMapper.window_schedule(9, 3, random.Random(6), final=True)
    assert set(sched) == {0, 1, 2}
    a = _mapper(torch, sc, frames, dev)
    a.capture_bank(_frames_of(frames[:2]), slots=3, loss_tap=True, fused_tail=True, capacity_margin=2.0)
    graph = a._bank.graph
    with pytest.raises(RuntimeError, match="holds no keyframe"):
        a.run_bank([2])
    f2 = frames[2]
    a.bank_set(2, gt_color=f2["gt_color"], gt_depth=f2["gt_depth"], render_mask=f2["render_mask"], settings=f2["settings"])
    assert a.run_bank(sched) == [] and a._bank.graph is graph
    b = _mapper(torch, sc, frames, dev)
    b.capture_bank(_frames_of(frames), loss_tap=True, fused_tail=True)
    assert b.run_bank(sched) == []
    _assert_same_training(torch, a, a._bank.graph, b, b._bank.graph)


def test_refresh_bank_equals_refresh_window(env):
    torch, _ = env
    from dqo_harness.fused_mapping import FusedMapper
    sc, frames, dev = _window_problem(torch, 3, 8)
    a, b = _mapper(torch, sc, frames, dev), _mapper(torch, sc, frames, dev)
    a.capture_bank(_frames_of(frames, own_tile_mask=True), loss_tap=True, fused_tail=True, capacity_margin=2.0)
    b.capture_window(_frames_of(frames, own_tile_mask=True), loss_tap=True, fused_tail=True, capacity_margin=2.0)
    for kw in (dict(global_opt=True, sample_ratio=0.3), dict()):  # the error branch, then the local one (whose masks the training uses)
        ra, rb = a.refresh_bank(**kw).clone(), b.refresh_window(**kw).clone()
        torch.cuda.synchronize()
        assert torch.equal(ra, rb) and bool(torch.isfinite(ra).all()) and 0 < float(ra.min())
        for k in range(3):
            assert torch.equal(a._bank.render_mask[k], b._frames[k].mask.view(a._bank.render_mask[k].shape)), (kw, k)
            assert torch.equal(a._bank.tile_mask[k], b._frames[k].tile_mask.view(a._bank.tile_mask[k].shape)), (kw, k)
            assert 0 < int(a._bank.tile_mask[k].sum()) and 0 < int(a._bank.render_mask[k].sum())
            if kw:  # (the error branch keeps 30 % of the tiles)
                assert int(a._bank.tile_mask[k].sum()) < a._bank.tile_mask[k].numel() and float(ra.max()) < 1
    sched = FusedMapper.window_schedule(8, 3, random.Random(8))
    assert a.run_bank(sched) == [] and b.run_window(sched) == 0
    _assert_same_training(torch, a, a._bank.graph, b, b._g)


def test_local_loop_with_the_object_gate_and_the_per_object_loss(env):
    from dqo_harness.fused_mapping import FusedMapper
    sched = FusedMapper.window_schedule(8, 3, random.Random(2))
    a, _ = _bank_against_window(env, sched, seed=9, gate=True)
    assert a._bank.gate and a._bank.graph.gate is not None and a.per_object_loss
