"""CPU: tests/traj_oracle.py — the numpy restatement of csrc/map_traj.hip — against values recorded from the reference's own functions
(tests/golden/traj_golden.npz, made by tests/golden/make_traj_golden.py), at the bars tests/test_gpu_traj.py holds the kernels to."""
import os

import numpy as np
import pytest

import traj_oracle as TO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHAINS = 3
ATE_BAR_CM = 1e-10  # coordinates below 10 m: a double rounding is ~1e-13 cm per coordinate; three orders over that
# prefixes the oracle is run on (every one is ~2 ms of Python): the degenerate ones, both sides of the 64-lane and the 256-thread
# boundary, and a spread of the rest.  The GPU test takes every prefix.
PREFIXES = sorted(set([1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 255, 256, 257] + list(range(10, 257, 37))))
DEGENERATE_FIT = ("line", "plane", "still")  # the optimum is not unique: only the error is compared


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "traj_golden.npz"))


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


def test_ate_prefixes_match_the_reference(gold):
    names = [str(n) for n in gold["ate_names"]]
    assert len(names) == 17 and gold[f"ate_{names[0]}_gt"].shape == (257, 3)
    worst = 0.0
    for name in names:
        gt, es, ref = gold[f"ate_{name}_gt"], gold[f"ate_{name}_es"], gold[f"ate_{name}_curve"]
        for i in PREFIXES:
            v, _, _ = TO.ate_prefix(gt[:i], es[:i])
            assert np.isfinite(v)
            worst = max(worst, abs(v - ref[i - 1]))
            assert abs(v - ref[i - 1]) <= ATE_BAR_CM, (name, i, v, ref[i - 1])
    print("oracle vs reference eval_ate, worst |difference|:", worst, "cm")
    assert np.all(gold["ate_same_curve"] < ATE_BAR_CM)


def test_fit_matches_align_where_it_is_unique(gold):
    for name in (str(n) for n in gold["ate_names"]):
        if name.startswith(DEGENERATE_FIT):
            continue
        _, R, t = TO.ate_prefix(gold[f"ate_{name}_gt"], gold[f"ate_{name}_es"])
        assert np.abs(R - gold[f"ate_{name}_rot"]).max() <= 1e-12 and np.abs(t - gold[f"ate_{name}_trans"]).max() <= 1e-12, name
        assert abs(np.linalg.det(R) - 1.0) < 1e-14


def _chain(gold, c, guf=1, **kw):
    tr = TO.Trajectory(12, projection=gold["projection"], gaussian_update_frame=guf,
                       init_pose=None if c != 2 else gold[f"chain{c}_init"], **kw)
    cams = []
    for i in range(12):
        tr.append(gold[f"chain{c}_rel"][i])
        cams.append(tr.cam)
    return tr, cams


def test_pose_chain_and_camera(gold):
    for c in range(CHAINS):
        tr, cams = _chain(gold, c)
        rel, ref = gold[f"chain{c}_rel"].astype(np.float64), gold[f"chain{c}_pose"]
        for i in range(1, 12):
            # the dot-product rounding bound for two 4-term sums, per entry
            bound = 8 * 2.0 ** -53 * (np.abs(tr.pose[i - 1]) @ np.abs(rel[i]))
            assert np.all(np.abs(tr.pose[i] - tr.pose[i - 1] @ rel[i]) <= bound)
        assert np.abs(tr.pose - ref).max() < 1e-14  # eleven products on: the two chains stay together
        for i in range(12):
            v64, f64 = gold[f"chain{c}_view64"][i], gold[f"chain{c}_full64"][i]
            cam = cams[i]
            assert np.all(np.abs(cam["c2w"] - ref[i]) <= ulp32(ref[i]))
            assert np.all(np.abs(cam["viewmatrix"] - v64) <= ulp32(v64))
            assert np.all(np.abs(cam["viewmatrix"] - gold[f"chain{c}_view"][i]) <= gold[f"chain{c}_view_dist"] + ulp32(v64))
            assert np.all(np.abs(cam["projmatrix"] - f64) <= ulp32(f64))
            assert np.all(np.abs(cam["projmatrix"] - gold[f"chain{c}_full"][i]) <= gold[f"chain{c}_full_dist"] + ulp32(f64))
            assert np.array_equal(cam["campos"], tr.pose[i][:3, 3].astype(np.float32))


def test_keyframe_metrics_and_decisions(gold):
    for c in range(CHAINS):
        # thresholds no row reaches: every row is compared against row 0, as the fixture's metrics are
        tr, _ = _chain(gold, c, theta_thres=1e9, trans_thres=1e9)
        assert tr.flags[0] == TO.TESTED | TO.LISTED and np.all(tr.flags[1:] == TO.TESTED) and tr.last_keyframe == 0
        assert np.abs(tr.kf_metric[1:, 0] - gold[f"chain{c}_theta"][1:]).max() <= 1e-9
        assert np.abs(tr.kf_metric[1:, 1] - gold[f"chain{c}_l2"][1:]).max() <= 1e-12
        # the reference's sequence of decisions with the fixture's thresholds: the keyframe row moves on with every keyframe
        th, tt = float(gold[f"chain{c}_theta_thres"]), float(gold[f"chain{c}_l2_thres"])
        tr, _ = _chain(gold, c, theta_thres=th, trans_thres=tt)
        kf = gold[f"chain{c}_seq_kf"]
        assert kf[1:].any() and not kf[1:].all()
        assert np.array_equal(tr.flags[1:], np.where(kf[1:], TO.TESTED | TO.KEYFRAME | TO.LISTED, TO.TESTED))
        assert np.abs(tr.kf_metric[1:, 0] - gold[f"chain{c}_seq_theta"][1:]).max() <= 1e-9
        assert np.abs(tr.kf_metric[1:, 1] - gold[f"chain{c}_seq_l2"][1:]).max() <= 1e-12
        assert tr.last_keyframe == int(np.nonzero(kf)[0][-1])
    tr, _ = _chain(gold, 0, guf=4, theta_thres=1e9, trans_thres=1e9)
    assert [i for i in range(12) if tr.flags[i] & TO.TESTED] == [0, 3, 7, 11]
    # identical poses are held to the decision only: the rotation is orthonormal to float32, so the cosine sits a rounding away from 1
    # and the angle is NaN, 0 or a few hundredths of a degree — all of them "no keyframe" at the smallest threshold of the fixture
    theta, l2 = TO.keyframe_metric(gold["same_pose"], gold["same_pose"])
    th = min(float(gold[f"chain{c}_theta_thres"]) for c in range(CHAINS))
    tt = min(float(gold[f"chain{c}_l2_thres"]) for c in range(CHAINS))
    assert not theta > th and not l2 > tt and not gold["same_theta"] > th and not gold["same_l2"] > tt


def test_overflow_leaves_the_store_alone(gold):
    tr = TO.Trajectory(12, gaussian_update_frame=1)
    for i in range(13):
        tr.append(gold["chain0_rel"][i % 12])
    assert tr.count == 12 and tr.overflow == 1


def test_world_maps(gold):
    for mi in range(2):
        v, n, M = gold[f"map{mi}_vertex_c"], gold[f"map{mi}_normal_c"], gold[f"map{mi}_c2w"]
        vw, nw = TO.world_maps(v, n, M)
        A = np.abs(M.astype(np.float64))
        for got, ref, src, t in ((vw, gold[f"map{mi}_vertex_w"], v, 1.0), (nw, gold[f"map{mi}_normal_w"], n, 0.0)):
            mag = np.abs(src.astype(np.float64)) @ A[:3, :3].T + t * A[:3, 3]
            assert got.dtype == np.float32 and np.all(np.abs(got.astype(np.float64) - ref) <= 8 * 2.0 ** -24 * mag)
        hole = (v == 0).all(-1)
        assert hole.any() and np.array_equal(vw[hole], np.broadcast_to(M[:3, 3], vw[hole].shape))
