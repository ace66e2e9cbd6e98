"""GPU: FusedMapper's row modes (set_training_rows: which rows a mapping call trains, which it renders) on EVERY entry path — the eager
step(), capture() + replay(), and a schedule that mixes them — each iteration teacher-forced against the CPU oracle iteration on the
rendered rows alone (test_gpu_window's machinery).  A hidden row (DQO_ROW_HIDDEN) is no Gaussian of the render: it must leave the image,
the loss and every trained row's gradient exactly as a map without it would; a frozen row (DQO_ROW_FROZEN) is rendered but not trained.

  mode           trainable        rendered
  all            all rows         all rows
  frozen         40 % random      all rows
  hidden         70 % "stable"    the same 70 %  (global_optimization, mapper.py:1105-1228)
  hidden_front   the rows behind  the rows behind; the hidden rows sit between them and the camera and cover most of the frame"""
import numpy as np
import pytest

import util_rast as U
from test_gpu_window import _finish_oracle, _oracle_iteration, _state, _window_problem, _check_iteration

pytestmark = pytest.mark.gpu

P = 20000
ITERS = 3
MODES = ("all", "frozen", "hidden", "hidden_front")
PATHS = {"step": ("step",) * ITERS, "replay": ("replay",) * ITERS, "mixed": ("replay", "step", "replay")}


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available()
    import _dqo_native
    _dqo_native.lib()
    from oracle import oracle_lib as ol
    return torch, ol


def _front_rows(sc, cam, rows, rng):
    """Move the Gaussians `rows` of scene `sc` (in place) between the camera and the room: 0.45-0.8 m in front of it, spread over the
    whole frustum, large and nearly opaque."""
    n = len(rows)
    z = rng.uniform(0.45, 0.8, n)
    u, v = rng.uniform(0, cam.W, n), rng.uniform(0, cam.H, n)
    pc = np.stack([(u - cam.cx) / cam.fx * z, (v - cam.cy) / cam.fy * z, z], 1)
    sc["xyz"][rows] = ((pc - cam.t) @ cam.Rw2c).astype(np.float32)  # x_w = Rw2c^T (x_c - t)
    sc["scales"][rows] = rng.uniform(0.01, 0.018, (n, 3)).astype(np.float32)
    sc["opacity"][rows] = np.float32(0.9)


_problems = {}


def _problem(torch, mode):
    """(scene, camera, frame, trainable [P] bool, rendered [P] bool) of a row mode; one frame of _window_problem's cfg-3 room."""
    if mode in _problems:
        return _problems[mode]
    sc, cams, frames, dev = _window_problem(torch, P, 1, seed=11)
    sc = {k: (np.array(v, copy=True) if isinstance(v, np.ndarray) else v) for k, v in sc.items()}
    rng = np.random.default_rng(21)
    everything = np.ones(P, bool)
    if mode == "all":
        trainable, rendered = everything, everything
    elif mode == "frozen":
        trainable, rendered = rng.uniform(size=P) < 0.4, everything
    elif mode == "hidden":
        trainable = rendered = rng.uniform(size=P) < 0.7
    else:
        front = rng.uniform(size=P) < 0.1
        _front_rows(sc, cams[0], np.nonzero(front)[0], rng)
        trainable = rendered = ~front
    _problems[mode] = (sc, cams[0], frames[0], dev, trainable, rendered)
    return _problems[mode]


def _sub(sc, rows):
    return {k: (v[rows] if isinstance(v, np.ndarray) and v.shape[:1] == (P,) else v) for k, v in sc.items()}


def _mapper(torch, sc, fr, dev, trainable, rendered, gate=None):
    from dqo_harness.fused_mapping import FusedMapper
    fm = FusedMapper(sc, fr["settings"], dev)
    if gate is not None:
        fm.set_object_gate(*gate)
    t = lambda a: torch.tensor(a, device=dev)
    fm.set_training_rows(trainable=t(trainable), rendered=t(rendered))
    fm.begin_mapping_call(reset_optimizer=True)
    return fm


def _iterate(torch, fm, fr, path, mask_u8):
    """One iteration of `path` ('step' / 'replay') under render mask mask_u8 (GPU uint8 [H, W]); returns the op's nine outputs."""
    if path == "step":
        return fm.step(fr["gt_color"], fr["gt_depth"], mask_u8)
    fm.set_frame(0, render_mask=mask_u8)
    out = fm.replay(frame=0)
    torch.cuda.synchronize()
    assert not fm.graph_overflowed()
    return out


def _check_forward(out, hr, rows):
    """The mapper's forward equals the eager op on the rendered rows alone: radii 0 on every other row, colour / depth / T bit for bit,
    hit maps after mapping the sub-scene's ids to map rows."""
    radii = out[8].cpu().numpy()
    hidden = np.ones(P, bool)
    hidden[rows] = False
    assert not radii[hidden].any(), f"{int((radii[hidden] != 0).sum())} hidden rows rendered"
    assert np.array_equal(radii[rows], hr.res["radii"])
    for i, k in ((0, "color"), (1, "depth"), (6, "T_map")):
        got = out[i].cpu().numpy()
        assert np.array_equal(got, hr.res[k]), (k, int((got != hr.res[k]).sum()), float(np.abs(got - hr.res[k]).max()))
    for i, k in ((2, "hit_color"), (3, "hit_depth")):
        h = hr.res[k]
        want = np.where(h >= 0, rows[np.clip(h, 0, None)], h)
        got = out[i].cpu().numpy()
        assert np.array_equal(got, want), (k, int((got != want).sum()))


def _run_against_oracle(torch, ol, fm, cam, fr, schedule, trainable, rendered, gate=None):
    """Teacher-forced: every iteration of `schedule` starts the oracle from the GPU's state; returns the per-iteration report."""
    if "replay" in schedule:
        fm.capture_window([fr], loss_tap=True, fused_tail=True)
        assert fm.step_count == 0
    init = dict(xyz=fm.init_xyz.cpu().numpy().astype(np.float64), scaling=fm.init_scaling.cpu().numpy().astype(np.float64),
                rotation=fm.init_rotation.cpu().numpy().astype(np.float64))
    rows = np.nonzero(rendered)[0]
    sub_of_row = np.full(P, -1)
    sub_of_row[rows] = np.arange(len(rows))
    trained = trainable & rendered
    attach_rows = fm.attach_mask.cpu().numpy().astype(bool)
    assert not attach_rows[~trained].any()
    gtc, gtd = fr["gt_color"].cpu().numpy(), fr["gt_depth"].cpu().numpy()
    base = fr["render_mask"].cpu().numpy().astype(bool)
    sub_gate = None if gate is None else (gate[0][rows], gate[1])
    report = []
    for it, path in enumerate(schedule):
        s0 = _state(fm)
        sca, out = _oracle_iteration(torch, ol, fm, cam, None, rows, s0, None, None, None, init, fm.lrs, gate=sub_gate)
        hr = U.HipRun(cam, sca, grad=False, object_gate=sub_gate)  # the eager op on the rendered rows alone
        names = U.HipRun.names
        bad = U.flipped_pixels(hr.res, {n: getattr(out["f32"][1], n) for n in names}, {n: getattr(out["f64"][1], n) for n in names})
        assert bad.mean() <= 1e-3
        mask = base & ~bad
        o = _iterate(torch, fm, fr, path, torch.tensor(mask, device=fm.device).to(torch.uint8))
        torch.cuda.synchronize()
        assert fm.step_count == it + 1
        _check_forward(o, hr, rows)
        s1 = _state(fm)
        loss, grads = _finish_oracle(ol, out, s0, rows, mask, gtc, gtd, init, attach_rows, pixel_object=None if gate is None else gate[1])
        np.testing.assert_allclose(fm.loss[:3].double().cpu().numpy(), loss, rtol=2e-5)
        _check_iteration(s0, s1, it + 1, trained, grads, fm.lrs, sub_of_row, report)
    if schedule[-1] == "replay":
        assert int(fm._step_dev.item()) == len(schedule) + 1
    return report


def test_hidden_front_rows_cover_most_of_the_frame(env):
    """The premise of the hidden_front mode: rendering the hidden rows by mistake changes most pixels of the frame."""
    torch, _ = env
    sc, cam, fr, dev, trainable, rendered = _problem(torch, "hidden_front")
    full = U.HipRun(cam, sc, grad=False).res["color"]
    part = U.HipRun(cam, _sub(sc, np.nonzero(rendered)[0]), grad=False).res["color"]
    changed = (np.abs(full - part) > 1e-3).any(0)
    assert changed.mean() > 0.5, float(changed.mean())


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("mode", MODES)
def test_row_mode_against_the_oracle(env, mode, path):
    """3 teacher-forced iterations of `path` in row mode `mode`: forward = the eager op on the rendered rows alone, loss and consumed
    gradient = the oracle's on those rows, Adam on the GPU's own moments, frozen / hidden rows bit for bit untouched."""
    torch, ol = env
    sc, cam, fr, dev, trainable, rendered = _problem(torch, mode)
    fm = _mapper(torch, sc, fr, dev, trainable, rendered)
    report = _run_against_oracle(torch, ol, fm, cam, fr, PATHS[path], trainable, rendered)
    print(mode, path, report)


@pytest.mark.parametrize("mode", MODES)
def test_eager_steps_match_replays(env, mode):
    """Two mappers with the same flags, mask and schedule, one stepping eagerly, one replaying: the same first forward bit for bit, and
    losses and states within test_graph_replay_matches_eager_steps' bar.  Not bitwise: the captured iteration forms its loss gradient in
    the blend kernels (loss tap) and its Adam step in the fused tail, with the bias corrections from the device-side step count — other
    kernels, other orders of summation; the eager step runs the separate loss and Adam kernels."""
    torch, _ = env
    sc, cam, fr, dev, trainable, rendered = _problem(torch, mode)
    a = _mapper(torch, sc, fr, dev, trainable, rendered)
    b = _mapper(torch, sc, fr, dev, trainable, rendered)
    b.capture_window([fr], loss_tap=True, fused_tail=True)
    for it in range(ITERS):
        oa = a.step(fr["gt_color"], fr["gt_depth"], fr["render_mask"])
        ob = b.replay(frame=0)
        torch.cuda.synchronize()
        if it == 0:
            for i in (0, 1, 2, 3, 6, 8):
                assert torch.equal(oa[i], ob[i]), i
    assert not b.graph_overflowed() and a.step_count == b.step_count == ITERS
    np.testing.assert_allclose(b.loss.cpu().numpy()[:3], a.loss.cpu().numpy()[:3], rtol=1e-5)
    still = torch.tensor(~(trainable & rendered), device=dev)
    for k, pa in a._params().items():
        pb = b._params()[k]
        assert torch.equal(pa[still], pb[still]), k
        lr = dict(xyz=0.001, shs=0.0005, opacity=1.0, scaling=0.004, rotation=0.001)[k]
        d = (pa - pb).abs()
        assert (d > 0.01 * lr + 1e-7).float().mean().item() < 1e-3, (k, d.max().item())
        for i in (0, 1):
            np.testing.assert_allclose(b.state[k][i].cpu().numpy(), a.state[k][i].cpu().numpy(), rtol=1e-3, atol=1e-9)
    assert torch.equal(a.confidence[still], b.confidence[still])


@pytest.mark.parametrize("path", ["step", "replay"])
def test_gated_mapper_hidden_rows_against_the_oracle(env, path):
    """The per-object job (set_object_gate, the bench path) in hidden mode: the per-object loss — the eager torch statement in step(),
    the loss tap in the graph — and its gradients are the gated oracle's on the rendered rows alone."""
    torch, ol = env
    sc, cam, fr, dev, trainable, rendered = _problem(torch, "hidden")
    go = np.asarray(sc["obj_id"], np.int32)
    hit = U.HipRun(cam, sc, grad=False).res["hit_depth"][0]
    po = np.where(hit >= 0, go[np.clip(hit, 0, None)], -1).astype(np.int32)
    assert len(np.unique(po[po >= 0])) >= 3
    fm = _mapper(torch, sc, fr, dev, trainable, rendered, gate=(go, po))
    assert fm.per_object_loss
    report = _run_against_oracle(torch, ol, fm, cam, fr, (path,) * ITERS, trainable, rendered, gate=(go, po))
    print("gated", path, report)


def test_hidden_rows_in_lazy_mode_are_the_exact_mode_bits(env):
    """step() in the 'lazy' sync mode (pooled contexts keyed by shape only, lists in per-tile buckets; the flags are read when the
    launches run) with the row flags rewritten in place between iterations — a hidden set, then another hidden set with frozen rows
    among the rendered ones: every forward, loss and state bit for bit what the same schedule gives in 'exact' mode, and the hidden rows
    of each iteration have radius 0."""
    torch, _ = env
    import diff_gaussian_rasterization_depth as dgr
    sc, cam, fr, dev, _, _ = _problem(torch, "hidden")
    rng = np.random.default_rng(31)
    s0, s1 = rng.uniform(size=P) < 0.7, rng.uniform(size=P) < 0.7
    sets = [(s0, s0), (s1 & (rng.uniform(size=P) < 0.4), s1)]  # (trainable, rendered)
    sched = [0, 0, 1, 1, 0]
    t = lambda a: torch.tensor(a, device=dev)
    runs = []
    try:
        for mode in ("lazy", "exact"):
            dgr.set_sync_mode(mode)
            fm = _mapper(torch, sc, fr, dev, *sets[0])
            rec = []
            for it, k in enumerate(sched):
                if it and k != sched[it - 1]:
                    fm.set_training_rows(trainable=t(sets[k][0]), rendered=t(sets[k][1]))
                out = fm.step(fr["gt_color"], fr["gt_depth"], fr["render_mask"])
                assert int(out[8][t(~sets[k][1])].abs().max().item()) == 0, (mode, it)
                rec.append(([o.clone() for o in out], fm.loss.clone()))
            dgr.verify_pending()
            torch.cuda.synchronize()
            runs.append((rec, _state(fm)))
    finally:
        dgr.set_sync_mode("exact")
    (lazy, s_lazy), (exact, s_exact) = runs
    for it, ((ol_, ll), (oe, le)) in enumerate(zip(lazy, exact)):
        for i in (0, 1, 2, 3, 4, 5, 6, 8):
            assert torch.equal(ol_[i], oe[i]), (it, i)
        assert torch.equal(ll[:3], le[:3]), it
    for k in ("xyz", "shs", "opacity", "scaling", "rotation", "conf", "live"):
        assert np.array_equal(s_lazy[k], s_exact[k]), k
    for k in s_lazy["m"]:
        assert np.array_equal(s_lazy["m"][k], s_exact["m"][k]) and np.array_equal(s_lazy["v"][k], s_exact["v"][k]), k
    assert not np.array_equal(s_exact["xyz"], sc["xyz"])  # (the schedule trained something)
