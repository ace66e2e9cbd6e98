"""GPU: pose corrections (csrc/map_repose.hip; dqo_icp.Trajectory.update_poses, dqo_icp.cameras_from_poses, FusedMapper.update_poses)
against dqo_traj_append's cameras byte for byte, against the numpy restatement (tests/repose_oracle.py), against values recorded from
the reference's Camera.updatePose (tests/golden/repose_golden.npz, the chains of traj_golden.npz), and as the trajectory -> window ->
bank chain against a twin mapper that was given the same cameras one frame at a time.

Bars: test_gpu_traj.py's — the camera tensors within one float32 ulp of the float64 truth, and within the reference's own recorded
distance from that truth plus that ulp of the reference's tensors; theta within 1e-9 degrees, l2 within 1e-12; everything else exact."""
import os

import numpy as np
import pytest

from dqo_harness import scenes
import repose_oracle as RO
import traj_oracle as TO

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "repose_golden.npz"))
GT = np.load(os.path.join(ROOT, "tests", "golden", "traj_golden.npz"))
CAMERA = ("c2w", "viewmatrix", "projmatrix", "campos")
# the fixture's 70 poses, then the three chains of traj_golden.npz (one projection serves both fixtures): pose, float64 truths, the
# reference's tensors and its own distances from the truth
POSES = np.concatenate([G["pose"]] + [GT[f"chain{c}_pose"] for c in range(3)])
VIEW64 = np.concatenate([G["view64"]] + [GT[f"chain{c}_view64"] for c in range(3)])
FULL64 = np.concatenate([G["full64"]] + [GT[f"chain{c}_full64"] for c in range(3)])
VIEW = np.concatenate([G["view"]] + [GT[f"chain{c}_view"] for c in range(3)])
FULL = np.concatenate([G["full"]] + [GT[f"chain{c}_full"] for c in range(3)])
VIEW_DIST = np.concatenate([np.full(70, G["view_dist"])] + [np.full(12, GT[f"chain{c}_view_dist"]) for c in range(3)])
FULL_DIST = np.concatenate([np.tile(G["full_dist"], (70, 1, 1))] + [np.tile(GT[f"chain{c}_full_dist"], (12, 1, 1)) for c in range(3)])
SENTINEL = -1515870811  # 0xA5A5A5A5 as int32


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import _dqo_native
    _dqo_native.lib()
    import dqo_icp
    assert np.array_equal(G["projection"], GT["projection"])
    return torch, dqo_icp


def cuda(torch, a):
    return torch.tensor(np.ascontiguousarray(a), device="cuda")


def np_(t):
    return t.detach().cpu().numpy()


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


def _rot(axis, deg):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    t = np.deg2rad(deg)
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * K @ K


_APPEND = {}


def append_cameras(torch, M):
    """What Trajectory.append(pose, relative=False) leaves for every pose of POSES: dict name -> [106, ...] (computed once)."""
    if not _APPEND:
        tr = M.Trajectory(len(POSES), "cuda", projection=cuda(torch, G["projection"]))
        poses = cuda(torch, POSES)
        got = {k: [] for k in CAMERA}
        for i in range(len(POSES)):
            tr.append(poses[i], relative=False)
            for k in CAMERA:
                got[k].append(getattr(tr, k).clone())
        _APPEND.update({k: np_(torch.stack(v)) for k, v in got.items()})
    return _APPEND


# ---- 1. the cameras are append's ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("T", [1, 63, 64, 65, 257])
def test_cameras_are_appends_bit_for_bit(env, T):
    torch, M = env
    ref = append_cameras(torch, M)
    rows = (np.arange(T) * 37 + T) % len(POSES)
    out = M.cameras_from_poses(cuda(torch, POSES), projection=cuda(torch, G["projection"]), rows=rows.tolist())
    assert set(out) == set(RO.FIELDS) | {"stats"} and np_(out["stats"]).tolist() == [0, T, 0, 0]
    got = {k: np_(out[k]) for k in RO.FIELDS}
    assert got["c2w"].shape == (T, 4, 4) and got["campos"].shape == (T, 3) and got["w2c"].dtype == np.float32
    for k in CAMERA:
        assert np.array_equal(got[k].view(np.int32), ref[k][rows].view(np.int32)), k  # byte for byte append's
    assert np.array_equal(got["w2c"].view(np.int32), ref["viewmatrix"][rows].transpose(0, 2, 1).copy().view(np.int32))
    for t, r in enumerate(rows):
        o = RO.cameras(POSES[r], G["projection"])
        for k in RO.FIELDS:
            assert np.array_equal(got[k][t], o[k]), (t, k)
        v64, f64 = VIEW64[r], FULL64[r]
        assert np.all(np.abs(got["viewmatrix"][t] - v64) <= ulp32(v64)), t
        assert np.all(np.abs(got["viewmatrix"][t] - VIEW[r]) <= VIEW_DIST[r] + ulp32(v64)), t
        assert np.all(np.abs(got["projmatrix"][t] - f64) <= ulp32(f64)), t
        assert np.all(np.abs(got["projmatrix"][t] - FULL[r]) <= FULL_DIST[r] + ulp32(f64)), t


def test_cameras_from_poses_defaults_out_and_other_dtypes(env):
    torch, M = env
    ref = append_cameras(torch, M)
    poses = cuda(torch, POSES)
    a = M.cameras_from_poses(poses)  # no projection: no projmatrix; all rows in order
    assert set(a) == {"c2w", "w2c", "viewmatrix", "campos", "stats"} and np_(a["stats"]).tolist() == [0, len(POSES), 0, 0]
    assert np.array_equal(np_(a["viewmatrix"]), ref["viewmatrix"]) and np.array_equal(np_(a["campos"]), ref["campos"])
    # a float32 stack is converted on the device first: the cameras of the ROUNDED poses
    b = M.cameras_from_poses(poses.float(), projection=cuda(torch, G["projection"]), rows=torch.tensor([5, 80], device="cuda"))
    for t, r in enumerate((5, 80)):
        o = RO.cameras(POSES[r].astype(np.float32).astype(np.float64), G["projection"])
        assert all(np.array_equal(np_(b[k])[t], o[k]) for k in RO.FIELDS)
    # out: written in place; a row outside the stack leaves its entry as it was and is counted
    keep = torch.full((3, 4, 4), 7.0, dtype=torch.float32, device="cuda")
    c = M.cameras_from_poses(poses, rows=[2, len(POSES), -1], out=dict(w2c=keep))
    assert c["w2c"] is keep and np_(c["stats"]).tolist() == [0, 1, 2, 0]
    assert np.array_equal(np_(keep)[0], ref["viewmatrix"][2].T) and bool((keep[1:] == 7.0).all())


# ---- 2. the store ------------------------------------------------------------------------------------------------------------------

def _trajectory(torch, M, cap=300, count=70, **kw):
    tr = M.Trajectory(cap, "cuda", projection=cuda(torch, G["projection"]), gaussian_update_frame=2, **kw)
    poses, gts = cuda(torch, G["pose"]), cuda(torch, G["pose"][::-1].copy())
    for i in range(count):
        tr.append(poses[i], relative=False, pose_gt=gts[i])
    return tr


def _corrected(n, seed=11):
    """n world poses that differ from the fixture's: its poses (cyclically) moved by a few centimetres and re-ordered."""
    rng = np.random.default_rng(seed)
    P = G["pose"][(np.arange(n) * 13 + 5) % 70].copy()
    P[:, :3, 3] += rng.uniform(-0.05, 0.05, size=(n, 3))
    return P


@pytest.mark.parametrize("n_new", [0, 1, 69, 70, 71, 300])
def test_store_semantics(env, n_new):
    torch, M = env
    cap, count = 300, 70
    tr = _trajectory(torch, M, cap, count)
    before = {k: np_(getattr(tr, k)).copy() for k in ("_pose", "_pose_gt", "flags", "kf_metric", "header")}
    assert before["flags"][:count].any() and before["_pose_gt"][:count].any() and before["header"].tolist()[0] == count
    new = _corrected(n_new)
    f32 = dict(dtype=torch.float32, device="cuda")
    # targets: rows -1, count and cap - 1 write nothing; row 3 twice, into different destinations
    dst = {k: torch.full((5,) + shape, 7.0, **f32) for k, shape in M.REPOSE_OUTPUTS}
    rows = [-1, count, cap - 1, 3, 3]
    table = M.repose_targets(rows, "cuda", **dst)
    stats = tr.update_poses(cuda(torch, new.reshape(n_new, 4, 4)), targets=table)
    torch.cuda.synchronize()
    n = min(count, n_new)
    assert np_(stats).tolist() == [n, 3, 3, 0]  # (written: the trajectory's own camera and row 3 twice)
    opose = before["_pose"].copy()
    outs, ostats = RO.repose(opose, count, new if n_new else None, [(count - 1, CAMERA)] + [(r, RO.FIELDS) for r in rows], G["projection"])
    assert ostats == [n, 3, 3, 0]
    pose = np_(tr._pose)
    assert np.array_equal(pose.view(np.int64), opose.view(np.int64))
    assert np.array_equal(pose[:n], new[:n]) and np.array_equal(pose[n:], before["_pose"][n:])
    for k in ("_pose_gt", "flags", "kf_metric", "header"):
        assert np.array_equal(np_(getattr(tr, k)), before[k]), k
    for k in CAMERA:  # the trajectory's own tensors follow row len - 1
        assert np.array_equal(np_(getattr(tr, k)), outs[0][k]), k
    for k, _ in M.REPOSE_OUTPUTS:
        got = np_(dst[k])
        assert (got[:3] == 7.0).all(), k
        assert np.array_equal(got[3], outs[4][k]) and np.array_equal(got[4], outs[5][k]), k
    assert len(tr) == count and np.array_equal(np_(tr.poses()), pose[:count])


def test_cameras_only_and_run_to_run(env):
    """new_poses None re-forms the cameras from the store; two calls on one input leave identical bytes everywhere."""
    torch, M = env
    res = []
    for _ in range(2):
        tr = _trajectory(torch, M, 80, 70)
        dst = {k: torch.zeros((70,) + shape, dtype=torch.float32, device="cuda") for k, shape in M.REPOSE_OUTPUTS}
        table = M.repose_targets(torch.arange(70, device="cuda"), "cuda", **dst)
        s0 = np_(tr.update_poses(None, targets=table)).tolist()
        first = {k: np_(v).copy() for k, v in dst.items()}
        s1 = np_(tr.update_poses(cuda(torch, _corrected(70)), targets=table)).tolist()
        assert s0 == [0, 71, 0, 0] and s1 == [70, 71, 0, 0]
        ref = append_cameras(torch, M)
        for k in CAMERA:
            assert np.array_equal(first[k], ref[k][:70]), k
        res.append((np_(tr._pose), {k: np_(v) for k, v in dst.items()}, {k: np_(getattr(tr, k)) for k in CAMERA}))
    assert np.array_equal(res[0][0].view(np.int64), res[1][0].view(np.int64))
    for a, b in ((res[0][1], res[1][1]), (res[0][2], res[1][2])):
        assert all(np.array_equal(a[k].view(np.int32), b[k].view(np.int32)) for k in a)


# ---- 3. unaligned destinations -----------------------------------------------------------------------------------------------------

def test_bank_rows_are_written_with_4_byte_stores_and_nothing_else(env):
    torch, M = env
    tr = _trajectory(torch, M, 16, 8)
    K = 5
    camera = torch.full((K, 40), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)
    bound = {0: 6, 2: 1, 4: 7}  # slot -> trajectory row
    base = camera.data_ptr()
    assert (base + 12) % 16 != 0  # a slot's viewmatrix is only 4-byte aligned
    entries = [(row, 0, 0, base + 160 * s + 12, base + 160 * s + 76, base + 160 * s + 140) for s, row in bound.items()]
    table = cuda(torch, np.asarray(entries, np.int64))
    new = _corrected(8, seed=5)
    stats = tr.update_poses(cuda(torch, new), targets=table)
    torch.cuda.synchronize()
    assert np_(stats).tolist() == [8, 4, 0, 0]
    got = np_(camera)
    for s in range(K):
        if s in bound:
            o = RO.cameras(new[bound[s]], G["projection"])
            assert np.array_equal(got[s, 3:19], o["viewmatrix"].reshape(-1)) and np.array_equal(got[s, 19:35], o["projmatrix"].reshape(-1))
            assert np.array_equal(got[s, 35:38], o["campos"])
            assert (got[s, :3].view(np.int32) == SENTINEL).all() and (got[s, 38:].view(np.int32) == SENTINEL).all(), s
        else:
            assert (got[s].view(np.int32) == SENTINEL).all(), s


# ---- 4. the keyframe test follows the correction -----------------------------------------------------------------------------------

def test_next_keyframe_test_compares_against_the_moved_keyframe(env):
    torch, M = env
    # check_keyframe compares the w2c sides (frame.R.T, frame.T): B is turned by 2 degrees and 0.2 m from A there, the corrected
    # keyframe A2 is 0.4 m from B
    wA = np.linalg.inv(G["pose"][10])
    wB, wA2 = wA.copy(), wA.copy()
    wB[:3, :3] = wA[:3, :3] @ _rot([0.3, -0.5, 0.8], 2.0)
    wB[:3, 3] += [0.2, 0.0, 0.0]
    wA2[:3, 3] -= [0.2, 0.0, 0.0]
    A, B, A2 = G["pose"][10].copy(), np.linalg.inv(wB), np.linalg.inv(wA2)
    theta_thres, trans_thres = 30.0, 0.3
    old, moved = TO.keyframe_metric(A, B), TO.keyframe_metric(A2, B)
    decide = lambda m: bool(m[0] > theta_thres or m[1] > trans_thres)
    assert not decide(old) and decide(moved) and moved[0] < theta_thres  # the decision differs, through the translation alone
    for correct, want in ((False, old), (True, moved)):
        tr = M.Trajectory(4, "cuda", gaussian_update_frame=1, keyframe_theta_thes=theta_thres, keyframe_trans_thes=trans_thres)
        tr.append(cuda(torch, A), relative=False)
        if correct:
            tr.update_poses(cuda(torch, A2[None]))
        tr.append(cuda(torch, B), relative=False)
        metric, flags = np_(tr.kf_metric), np_(tr.flags)
        assert abs(metric[1, 0] - want[0]) <= 1e-9 and abs(metric[1, 1] - want[1]) <= 1e-12, (correct, metric[1], want)
        assert tr.is_keyframe() == decide(want) and flags[0] == TO.TESTED | TO.LISTED
        assert flags[1] == (TO.TESTED | TO.KEYFRAME | TO.LISTED if decide(want) else TO.TESTED)
        assert np_(tr.header).tolist() == [2, 1 if decide(want) else 0, 0, 0]
        assert np.array_equal(np_(tr.poses())[0], A2 if correct else A)


# ---- 5, 6. the bank and the window -------------------------------------------------------------------------------------------------

N_KEY = 5
_PROBLEM = {}


def _small_cameras():
    return [scenes.replica_camera(W=64, H=48, fx=32.0, fy=32.0, cx=31.5, cy=23.5, yaw=12.0 + 3.5 * k, pitch=4.0 - 1.5 * k,
                                  pos=(0.3 + 0.15 * k, 0.1 - 0.03 * k, -1.85 + 0.12 * k)) for k in range(N_KEY)]


def _problem(torch):
    """Five 48x64 keyframes of a 3000-Gaussian room (tests/test_gpu_window_bank.py's recipe), their world poses, and the corrected
    poses: every camera moved by a centimetre or two and turned by half a degree.  Computed once and left unchanged."""
    if not _PROBLEM:
        from dqo_harness import mapping
        _, sc = scenes.make_config(3, P=3000)
        dev = torch.device("cuda")
        cams, frames = _small_cameras(), []
        for k, cam in enumerate(cams):
            st = mapping.make_settings(cam, dev)
            tgt = mapping.perturbed_target(sc, st, dev, 300 + 7 * k)
            rng = np.random.default_rng(60 + k)
            mask = torch.tensor(rng.uniform(size=(cam.H, cam.W)) < 0.8, device=dev) & (tgt["pix_obj"] >= 0)
            frames.append(dict(settings=st, gt_color=tgt["gt_color"].contiguous(), gt_depth=tgt["gt_depth"].contiguous(),
                               render_mask=mask.to(torch.uint8).contiguous()))
        poses = np.stack([np.linalg.inv(cam.Rt) for cam in cams])
        rng = np.random.default_rng(9)
        new = poses.copy()
        for k in range(N_KEY):
            new[k, :3, :3] = poses[k, :3, :3] @ _rot(rng.normal(size=3), 0.5)
            new[k, :3, 3] += rng.uniform(-0.02, 0.02, size=3)
        _PROBLEM.update(sc=sc, frames=frames, dev=dev, poses=poses, new=new, projection=cams[0].projection_matrix.copy())
    p = _PROBLEM
    return p["sc"], p["frames"], p["dev"], p["poses"], p["new"], p["projection"]


def _frames_of(frames, rows=False):
    return [dict({k: (v if k == "settings" else v.clone()) for k, v in fr.items()}, **({"row": i} if rows else {})) for i, fr in enumerate(frames)]


def _mapper(sc, frames, dev):
    from dqo_harness.fused_mapping import FusedMapper
    fm = FusedMapper(sc, frames[0]["settings"], dev)
    fm.begin_mapping_call(reset_optimizer=True)
    return fm


def _traj_of(torch, M, poses, projection, cap=8):
    tr = M.Trajectory(cap, "cuda", projection=cuda(torch, projection))
    P = cuda(torch, poses)
    for i in range(len(poses)):
        tr.append(P[i], relative=False)
    return tr


def _settings_by_append(torch, M, pose, projection, template):
    """The path without the operator: append(relative=False) on a scratch trajectory, and its settings."""
    scratch = M.Trajectory(1, "cuda", projection=cuda(torch, projection))
    scratch.append(cuda(torch, pose), relative=False)
    return scratch.settings(template)


def _assert_same_training(torch, a, ga, b, gb):
    torch.cuda.synchronize()
    for k in a._params():
        assert torch.equal(a._params()[k], b._params()[k]), k
        assert torch.equal(a.state[k][0], b.state[k][0]) and torch.equal(a.state[k][1], b.state[k][1]), k
    assert torch.equal(a.confidence, b.confidence) and torch.equal(a.loss, b.loss)
    assert a.step_count == b.step_count and int(a._step_dev.item()) == int(b._step_dev.item()) == a.step_count + 1
    for i, (x, y) in enumerate(zip(ga.out, gb.out)):
        assert torch.equal(x, y), i


def test_bank_follows_a_correction(env):
    torch, M = env
    import _dqo_native as N
    sc, frames, dev, poses, new, projection = _problem(torch)
    a = _mapper(sc, frames, dev)
    a.capture_bank(_frames_of(frames, rows=True), loss_tap=True, fused_tail=True, capacity_margin=2.0)
    bank, g = a._bank, a._bank.graph
    assert bank.rows == list(range(N_KEY))
    tr = _traj_of(torch, M, poses, projection)
    # schedule [0, 0]: one iteration, a changed pose for slot 0, the second iteration
    with torch.cuda.device(dev):
        bank.schedule[:2].copy_(cuda(torch, np.zeros((2, 2), np.int32)))
        bank.arm(2, N.current_stream())
    a._bank_launch(1)
    torch.cuda.synchronize()
    assert int(bank.word("force")) == 0 and int(bank.word("cursor")) == 1
    first = {k: getattr(g.settings, k).clone() for k in ("viewmatrix", "projmatrix", "campos")}
    moved = poses.copy()
    moved[0] = new[0]
    stats = a.update_poses(tr, cuda(torch, moved[:1]))  # (rows beyond n_new keep their pose: the other slots' cameras are formed from the store)
    torch.cuda.synchronize()
    assert np_(stats).tolist() == [1, N_KEY + 1, 0, 0] and int(bank.word("force")) == 1
    assert all(torch.equal(getattr(g.settings, k), first[k]) for k in first)  # the staged camera moves with the select, not before
    a._bank_launch(1)
    torch.cuda.synchronize()
    assert int(bank.word("force")) == 0 and int(bank.word("cursor")) == 2 and int(bank.word("overrun")) == 0
    o = RO.cameras(new[0], projection)
    for k in ("viewmatrix", "projmatrix", "campos"):
        assert np.array_equal(np_(getattr(g.settings, k)).reshape(-1), o[k].reshape(-1)), k
        assert not torch.equal(getattr(g.settings, k), first[k]), k
    assert np.array_equal(np_(tr.poses()), moved)
    row = np_(bank.camera)
    for s in range(N_KEY):
        o = RO.cameras(moved[s], projection)
        assert np.array_equal(row[s, 3:19], o["viewmatrix"].reshape(-1)) and np.array_equal(row[s, 35:38], o["campos"])
        assert (row[s, :3] == 0).all() and (row[s, 38:] == 0).all()


def test_run_bank_after_a_correction_equals_the_per_slot_path(env):
    torch, M = env
    sc, frames, dev, poses, new, projection = _problem(torch)
    sched = [0, 3, 1, (2, 4), 4, 0, 2, 3]
    a, b = _mapper(sc, frames, dev), _mapper(sc, frames, dev)
    a.capture_bank(_frames_of(frames, rows=True), loss_tap=True, fused_tail=True, capacity_margin=2.0)
    b.capture_bank(_frames_of(frames), loss_tap=True, fused_tail=True, capacity_margin=2.0)
    tr = _traj_of(torch, M, poses, projection)
    a.update_poses(tr, cuda(torch, new))
    for k in range(N_KEY):
        b.bank_set(k, settings=_settings_by_append(torch, M, new[k], projection, frames[k]["settings"]))
    torch.cuda.synchronize()
    assert torch.equal(a._bank.camera, b._bank.camera) and np.array_equal(np_(tr.poses()), new)
    assert a.run_bank(sched) == [] and b.run_bank(sched) == []
    assert a.step_count == len(sched)
    _assert_same_training(torch, a, a._bank.graph, b, b._bank.graph)


def test_window_after_a_correction_equals_the_per_frame_path(env):
    torch, M = env
    sc, frames, dev, poses, new, projection = _problem(torch)
    n = 3
    sched = [0, 2, 1, 1, 0, 2]
    a, b = _mapper(sc, frames, dev), _mapper(sc, frames, dev)
    fa = _frames_of(frames[:n], rows=True)
    fa[1].pop("row")
    a.capture_window(fa, loss_tap=True, fused_tail=True, capacity_margin=2.0)
    a.set_frame(1, row=1)  # bound after the capture
    b.capture_window(_frames_of(frames[:n]), loss_tap=True, fused_tail=True, capacity_margin=2.0)
    assert a._frame_rows == {0: 0, 1: 1, 2: 2}
    tr = _traj_of(torch, M, poses, projection)
    stats = a.update_poses(tr, cuda(torch, new))
    for k in range(n):
        b.set_frame(k, settings=_settings_by_append(torch, M, new[k], projection, frames[k]["settings"]))
    torch.cuda.synchronize()
    assert np_(stats).tolist() == [N_KEY, n + 1, 0, 0]
    for k in range(n):
        for name in ("viewmatrix", "projmatrix", "campos", "bg"):
            assert torch.equal(getattr(a._frames[k].settings, name), getattr(b._frames[k].settings, name)), (k, name)
    table = a._repose_table
    a.update_poses(tr)  # the table is kept while nothing is bound or captured; a new binding drops it
    assert a._repose_table is table
    assert a.run_window(sched) == 0 and b.run_window(sched) == 0
    _assert_same_training(torch, a, a._g, b, b._g)
    # the refusals, before any launch
    before = np_(tr._pose).copy()
    a.set_frame(2, row=4)
    assert a._repose_table is None
    keep = a._frames[2]
    a._frames[2] = a._frames[0]  # one set of camera tensors under rows 0 and 4
    with pytest.raises(ValueError, match="rows 0 and 4"):
        a.update_poses(tr, cuda(torch, poses))
    a._frames[2] = keep
    keep_settings = keep.settings
    keep.settings = a.settings  # a graph on the mapper's default camera tensors
    with pytest.raises(ValueError, match="default camera"):
        a.update_poses(tr, cuda(torch, poses))
    keep.settings = keep_settings
    torch.cuda.synchronize()
    assert np.array_equal(np_(tr._pose), before)
    no_proj = M.Trajectory(2, "cuda")
    with pytest.raises(ValueError, match="projection"):
        a.update_poses(no_proj)


# ---- 7. captured -------------------------------------------------------------------------------------------------------------------

def test_update_poses_replayed_from_one_graph(env):
    torch, M = env
    sets = [_corrected(70, seed=21), _corrected(70, seed=22)]
    eager = []
    for new in sets:
        tr = _trajectory(torch, M, 80, 70)
        tr.update_poses(cuda(torch, new))
        eager.append((np_(tr._pose), {k: np_(getattr(tr, k)) for k in CAMERA}))
    tr = _trajectory(torch, M, 80, 70)
    static = cuda(torch, _corrected(70, seed=20))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        tr.update_poses(static)
    for new, (pose, cam) in zip(sets, eager):
        static.copy_(cuda(torch, new))
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(np_(tr._pose).view(np.int64), pose.view(np.int64))
        assert np_(tr.repose_stats).tolist() == [70, 1, 0, 0]
        for k in CAMERA:
            assert np.array_equal(np_(getattr(tr, k)).view(np.int32), cam[k].view(np.int32)), k
