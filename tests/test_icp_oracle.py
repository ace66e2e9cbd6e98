"""CPU: the order-exact ICP oracle (tests/icp_oracle.py) against the goldens of the reference's own SLAM/icp.py, the preconditions of
the scenes the GPU tests run (tests/icp_scenes.py), and the branch of the Gauss-Newton solve each solve scene is named for."""
import numpy as np
import pytest

import icp_oracle as O
import icp_scenes as S
from oracle import map_oracle as mo
from test_oracle_icp import CASES, DIST_THR, G, NORMAL_THR, case


def golden_sums(c):
    v0, v1, n0, n1, pose, K = case(c)
    ok, J, r = O.per_pixel(v0, v1, n0, n1, pose, *O.intrinsics(K), DIST_THR, NORMAL_THR)
    return ok, O.sums(ok, J, r)


@pytest.mark.parametrize("c", CASES)
def test_valid_mask_is_the_references(c):
    ok, _ = golden_sums(c)
    assert int((ok != G[f"{c}_valid"]).sum()) == 0


@pytest.mark.parametrize("c", CASES)
def test_sums_within_the_references_own_fp32_summation(c):
    """The goldens are fp32 sums of n fp32 terms in an order of torch's choosing: off the exact sum by at most n * 2^-24 * sum|term|
    (plus the final rounding, one ulp).  Seen: at most 3.3e-6 per entry of JtJ and 5.0e-6 per entry of JtR."""
    _, (JtJ, JtR, n, absJ, absR) = golden_sums(c)
    gJ, gR = G[f"{c}_JtJ"], G[f"{c}_JtR"].reshape(-1)
    assert n == int(G[f"{c}_valid"].sum())
    assert (np.abs(JtJ.astype(np.float64) - gJ) <= n * 2.0 ** -24 * absJ + np.spacing(np.abs(gJ))).all()
    assert (np.abs(JtR.astype(np.float64) - gR) <= n * 2.0 ** -24 * absR + np.spacing(np.abs(gR))).all()


@pytest.mark.parametrize("c", CASES)
def test_old_and_new_oracle_agree_on_the_mask(c):
    v0, v1, n0, n1, pose, K = case(c)
    ok, _ = golden_sums(c)
    assert np.array_equal(ok, mo.icp_normal_equations(v0, v1, n0, n1, pose, K, DIST_THR, NORMAL_THR)[2])


def test_probe_is_one_term_of_the_sums():
    sc = S.sweep_scene(17, 23)
    t = S.trace(sc)
    px = tuple(np.argwhere(t["ok"])[5])
    one = np.zeros_like(t["ok"])
    one[px] = True
    JtJ, JtR, n = O.probe(t["ok"], t["J"], t["r"], px)
    sJ, sR, sn, _, _ = O.sums(one, t["J"], t["r"])
    assert n == sn == 1 and np.array_equal(JtJ, sJ) and np.array_equal(JtR, sR)
    assert O.probe(t["ok"], t["J"], t["r"], tuple(np.argwhere(~t["ok"])[0]))[2] == 0


@pytest.mark.parametrize("size", S.SWEEP_SIZES)
def test_sweep_scene_preconditions(size):
    S.check_sweep(S.sweep_scene(*size))
    assert size != (513, 512) or size[0] * size[1] > 1024 * 256 >= 340 * 600


@pytest.mark.parametrize("tx", S.EDGE_TX)
@pytest.mark.parametrize("with_nan", [True, False])
def test_edge_scene_preconditions(tx, with_nan):
    S.check_edge(S.edge_scene(tx, with_nan), tx, with_nan)


def step(sc, damping, pose=None):
    return O.gauss_newton_step(sc["pose"] if pose is None else pose, sc["v0"], sc["v1"], sc["n0"], sc["n1"], sc["K"], 1.0, sc["thr_d"],
                                sc["thr_n"], damping)


def test_rank3_scene_fails_cholesky_at_pivot_2_and_rotates():
    sc = S.rank3_scene()
    pose = sc["pose"]
    for _ in range(3):  # the rank stays 3 along the iterations: frame 1's normals are (0, 0, 1) whatever the pose
        out, n, info = step(sc, 0.0, pose)
        H = info["H"]
        assert n > 30 and info["pivot"] == 2 and info["branch"] == "pinv"
        assert not H[2:5].any() and not H[:, 2:5].any() and np.linalg.matrix_rank(H.astype(np.float64)) == 3
        assert H[0, 1] != 0 and H[0, 5] != 0 and H[1, 5] != 0  # coupled: the Jacobi sweeps have to rotate
        assert info["theta"] > 1e-4 and np.abs(info["xi"][:2]).min() > 1e-5 and abs(info["xi"][5]) > 1e-3
        assert np.isfinite(out).all() and not np.array_equal(out, pose)
        pose = out


def test_rank1_scene_branches():
    sc = S.rank1_scene()
    t = S.trace(sc)
    assert t["ok"].sum() == 1 and t["ok"][2, 3]
    assert np.array_equal(t["J"][2, 3], np.array([0, 0, 0, 0, 0, 1], np.float32)) and t["r"][2, 3] == np.float32(-0.125)
    out, n, info = step(sc, 0.0)
    want = np.eye(4, dtype=np.float32)
    want[2, 3] = 0.125
    assert n == 1 and info["pivot"] == 0 and info["branch"] == "pinv" and info["theta"] <= 1e-8
    assert np.array_equal(out, want)  # through the small-angle branch of exp_se3 with a translation
    out, n, info = step(sc, 1e-4)
    assert n == 1 and info["pivot"] is None and info["branch"] == "cholesky" and info["theta"] <= 1e-8
    assert 0.12499 > out[2, 3] > 0.12498  # 0.125 / (1 + 1e-4)


@pytest.mark.parametrize("damping", [1e-6, 1e-4])
def test_fullrank_scene_goes_through_cholesky(damping):
    sc = S.sweep_scene(17, 23)
    out, n, info = step(sc, damping)
    assert n > 100 and info["pivot"] is None and info["branch"] == "cholesky" and info["theta"] > 1e-8
    assert np.linalg.matrix_rank(info["H"].astype(np.float64)) == 6


@pytest.mark.parametrize("damping", [0.0, 1e-6])
def test_overflow_scene_is_non_finite_and_keeps_the_pose(damping):
    sc = S.overflow_scene()
    t = S.trace(sc)
    JtJ, JtR, n, _, _ = O.sums(t["ok"], t["J"], t["r"])
    assert n == S.trace(S.sweep_scene(17, 23))["ok"].sum() and np.isinf(JtJ).any() and np.isfinite(JtR).all()
    out, n2, info = step(sc, damping)
    assert n2 == n and info["branch"] == "nonfinite" and info["pivot"] == 0
    assert np.isnan(info["H"]).any() == (damping == 0.0)
    assert out.tobytes() == sc["pose"].tobytes()


def test_nan_residual_scene_gives_a_nan_pose_like_the_reference():
    """That the reference's pose is NaN here is read from SLAM/icp.py (inverse of a finite H times a NaN right-hand side); no golden
    records it."""
    sc = S.nan_residual_scene()
    out, n, info = step(sc, 1e-6)
    assert n == S.trace(S.sweep_scene(17, 23))["ok"].sum() and info["branch"] == "cholesky"
    assert np.isnan(out[:3]).all() and np.array_equal(out[3], [0, 0, 0, 1])
