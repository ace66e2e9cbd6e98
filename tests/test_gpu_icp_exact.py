"""GPU: csrc/icp.hip against the order-exact oracle (tests/icp_oracle.py) on the scenes of tests/icp_scenes.py.

Per pixel: with frame-0 depth at one pixel only, dqo_icp_normal_equations returns that pixel's J J^T, J r and mask, which must equal the
oracle's bit for bit.  Whole images: the count must be equal and every sum within one fp32 ulp plus the bound of its own fp64
accumulation.  dqo_icp_gauss_newton (intrinsics K * k_scale read on the device, solve on the device) must return the oracle's count
and the oracle's pose on every branch of its solve."""
import numpy as np
import pytest

import icp_oracle as O
import icp_scenes as S

pytestmark = pytest.mark.gpu

EDGE_CASES = [("edge", tx, False) for tx in S.EDGE_TX] + [("edge", 0.125, True)]
IMAGE_CASES = [("sweep",) + s for s in S.SWEEP_SIZES] + EDGE_CASES + [("overflow",), ("nan_residual",)]
_SCENES, _SUMS = {}, {}


def scene(key):
    """The scene of a case, built once and shared (read only)."""
    if key not in _SCENES:
        kind = key[0]
        sc = (S.sweep_scene(*key[1:]) if kind == "sweep" else S.edge_scene(*key[1:]) if kind == "edge" else
              dict(overflow=S.overflow_scene, nan_residual=S.nan_residual_scene, rank3=S.rank3_scene, rank1=S.rank1_scene)[kind]())
        _SCENES[key] = sc
    return _SCENES[key]


def oracle_sums(key):
    """(trace, sums) of the oracle at the scene's own pose and intrinsics, computed once."""
    if key not in _SUMS:
        t = S.trace(scene(key))
        _SUMS[key] = t, O.sums(t["ok"], t["J"], t["r"])
    return _SUMS[key]


@pytest.fixture(scope="module")
def icp():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import _dqo_native
    _dqo_native.lib()
    import dqo_icp
    return torch, dqo_icp


def maps_on_gpu(torch, sc):
    return [torch.tensor(sc[k], device="cuda") for k in ("v0", "v1", "n0", "n1")]


def normal_equations(torch, M, sc, maps=None):
    v0, v1, n0, n1 = maps or maps_on_gpu(torch, sc)
    return M.normal_equations(v0, v1, n0, n1, torch.tensor(sc["pose"], device="cuda"), torch.tensor(sc["K"]), sc["thr_d"], sc["thr_n"])


def same_bits(got, want):
    """Equal bit for bit; NaN must sit in the same places (its payload is not compared)."""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.int32)[~nan], want.view(np.int32)[~nan])


def gauss_newton(icp, sc, pose, damping, K=None, k_scale=1.0, iters=1, maps=None):
    """`iters` dqo_icp_gauss_newton calls on a device pose; yields (pose before, pose after, count) of each as numpy."""
    torch, N = icp[0], icp[1].N
    lib = N.lib()
    p = torch.tensor(np.asarray(pose, np.float32), device="cuda").contiguous()
    cnt = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    ws = torch.empty(lib.dqo_icp_workspace_bytes(), dtype=torch.uint8, device="cuda")
    t = maps or maps_on_gpu(torch, sc)
    Kd = torch.tensor(np.asarray(sc["K"] if K is None else K, np.float32), device="cuda")
    H, W = sc["v0"].shape[:2]
    for _ in range(iters):
        before = p.cpu().numpy()
        N.check(lib.dqo_icp_gauss_newton(H, W, *[N.ptr(a) for a in t], N.ptr(p), N.ptr(Kd), float(k_scale), float(sc["thr_d"]),
                                         float(sc["thr_n"]), float(damping), N.ptr(cnt), N.ptr(ws), ws.numel(), N.current_stream()))
        yield before, p.cpu().numpy(), int(cnt.cpu()[0])


def oracle_step(sc, pose, damping, K=None, k_scale=1.0):
    return O.gauss_newton_step(pose, sc["v0"], sc["v1"], sc["n0"], sc["n1"], sc["K"] if K is None else K, k_scale, sc["thr_d"], sc["thr_n"],
                               damping)


def pose_tol(want):
    """One fp32 rounding of each of the four entries of T's row plus the product's four adds: 8 * 2^-24 of the largest magnitude."""
    return 8 * 2.0 ** -24 * max(1.0, float(np.abs(want).max()))


def assert_pose_close(got, want, what):
    err = float(np.abs(got.astype(np.float64) - want).max())
    print(f"{what}: max |pose - oracle| = {err:.3e}, bound {pose_tol(want):.3e}")
    assert np.isfinite(got).all() and err <= pose_tol(want), what


# ---- per pixel ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", [("sweep", 17, 23)] + [("edge", tx, True) for tx in S.EDGE_TX], ids=str)
def test_probe_every_pixel_bitwise(icp, key):
    torch, M = icp
    sc = scene(key)
    t, _ = oracle_sums(key)
    H, W = t["ok"].shape
    v0, v1, n0, n1 = maps_on_gpu(torch, sc)
    lone = torch.zeros_like(v0)
    outs = []
    for i in range(H):
        for j in range(W):
            lone[i, j] = v0[i, j]
            JtJ, JtR, cnt = normal_equations(torch, M, sc, (lone, v1, n0, n1))
            outs.append(torch.cat([JtJ.reshape(-1), JtR.reshape(-1), cnt.reshape(1).float()]))
            lone[i, j] = 0
    got = torch.stack(outs).cpu().numpy()
    want = np.stack([np.concatenate([a.reshape(-1), b, [np.float32(n)]]) for a, b, n in
                     (O.probe(t["ok"], t["J"], t["r"], (i, j)) for i in range(H) for j in range(W))]).astype(np.float32)
    assert np.array_equal(got[:, 42], want[:, 42]), f"mask differs at pixels {np.nonzero(got[:, 42] != want[:, 42])[0][:8]} (row-major)"
    for k in range(H * W):
        assert same_bits(got[k], want[k]), f"pixel {divmod(k, W)}: got {got[k]}, oracle {want[k]}"
    assert want[:, 42].sum() > 0


# ---- whole images ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", IMAGE_CASES, ids=str)
def test_whole_image_count_equal_sums_within_accumulation_bound(icp, key):
    """Seen on MI355X: the largest distance is 0 fp32 ulp on every case (bound: 1 ulp + n * 2^-53 * sum|term|)."""
    torch, M = icp
    sc = scene(key)
    _, (oJ, oR, n, absJ, absR) = oracle_sums(key)
    maps = maps_on_gpu(torch, sc)
    JtJ, JtR, cnt = normal_equations(torch, M, sc, maps)
    JtJ2, JtR2, cnt2 = normal_equations(torch, M, sc, maps)
    assert torch.equal(cnt, cnt2) and same_bits(JtJ2.cpu().numpy(), JtJ.cpu().numpy()) and same_bits(JtR2.cpu().numpy(), JtR.cpu().numpy())
    JtJ, JtR = JtJ.cpu().numpy(), JtR.cpu().numpy().reshape(-1)
    assert int(cnt) == n
    assert same_bits(JtJ, JtJ.T)
    for got, want, absum in ((JtJ, oJ, absJ), (JtR, oR, absR)):
        fin = np.isfinite(want)
        assert same_bits(np.where(fin, 0, got), np.where(fin, 0, want))  # inf and NaN where the oracle has them, and nowhere else
        ulp = np.spacing(np.abs(want[fin])).astype(np.float64)
        err = np.abs(got[fin].astype(np.float64) - want[fin])
        bound = ulp + n * 2.0 ** -53 * absum[fin]
        if err.size:
            print(f"{key}: n = {n}, largest |sum - oracle| = {float((err / ulp).max()):.2f} ulp, bound there {float((bound / ulp)[np.argmax(err / ulp)]):.2f} ulp")
        assert (err <= bound).all(), (key, got, want)


# ---- the device-K variant ----------------------------------------------------------------------------------------------------------
KDEV_SCENES = [("sweep",) + s for s in S.SWEEP_SIZES] + [("edge", tx, False) for tx in S.EDGE_TX]


@pytest.mark.parametrize("k_scale", [1.0, 0.5, 0.25, 0.3])
@pytest.mark.parametrize("key", KDEV_SCENES, ids=str)
def test_gauss_newton_reads_K_times_scale_on_the_device(icp, key, k_scale):
    """The tracker's variant, on every sweep size and the edge scene at each tx: the full-resolution K lives in device memory and is
    scaled in the kernel.  K is the scene's divided by k_scale in fp32, so the products are the scene's intrinsics up to their
    rounding, which the oracle repeats (at 0.5 and 0.25 they are the scene's exactly, so the edge pixels stay on their comparisons)."""
    sc = scene(key)
    K = (sc["K"] / np.float32(k_scale)).astype(np.float32)
    K[2, 2] = 1
    want, n, info = oracle_step(sc, sc["pose"], 1e-4, K, k_scale)
    assert n > 0 and info["branch"] == "cholesky"
    if k_scale in (1.0, 0.5, 0.25):
        assert n == oracle_sums(key)[1][2]
    (before, after, cnt), = gauss_newton(icp, sc, sc["pose"], 1e-4, K, k_scale)
    assert cnt == n
    assert_pose_close(after, want, f"{key} k_scale {k_scale}")


# ---- every branch of the device-side solve -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("damping,branch", [(0.0, "pinv"), (1e-4, "cholesky")])
def test_rank1_solve_bitwise(icp, damping, branch):
    sc = scene(("rank1",))
    want, n, info = oracle_step(sc, sc["pose"], damping)
    assert n == 1 and info["branch"] == branch and info["theta"] <= 1e-8
    (before, after, cnt), = gauss_newton(icp, sc, sc["pose"], damping)
    assert cnt == 1
    # bitwise although the kernel substitutes through L (r / sqrt(d) / sqrt(d)) and the oracle solves by LU: H is diagonal, xi is
    # 0.125 or 0.125 / (1 + eps) to a few fp64 ulps either way, and T rounds it to fp32 nowhere near a tie
    assert same_bits(after, want), (after, want)


@pytest.mark.parametrize("key,damping,branch", [(("rank3",), 0.0, "pinv"), (("sweep", 17, 23), 1e-6, "cholesky"),
                                                (("sweep", 17, 23), 1e-4, "cholesky")], ids=str)
def test_three_chained_iterations_vs_oracle(icp, key, damping, branch):
    """Three device iterations in a row; each is held against the oracle's step from the pose it started from, which is what the
    one-step bound is derived for."""
    sc = scene(key)
    for it, (before, after, cnt) in enumerate(gauss_newton(icp, sc, sc["pose"], damping, iters=3)):
        want, n, info = oracle_step(sc, before, damping)
        assert info["branch"] == branch and (branch != "pinv" or info["pivot"] == 2)
        assert cnt == n and n > 30
        assert_pose_close(after, want, f"{key} damping {damping} iteration {it}")
        assert not np.array_equal(after, before)


@pytest.mark.parametrize("damping", [0.0, 1e-6])
def test_non_finite_normal_equations_leave_the_pose(icp, damping):
    sc = scene(("overflow",))
    want, n, info = oracle_step(sc, sc["pose"], damping)
    assert info["branch"] == "nonfinite" and same_bits(want, sc["pose"])
    (before, after, cnt), = gauss_newton(icp, sc, sc["pose"], damping)
    assert cnt == n
    assert same_bits(after, sc["pose"]), after


def test_nan_residual_gives_the_references_nan_pose(icp):
    """NaN in the same places as the oracle's pose, and the last row kept.  That the reference's pose is NaN here is read from
    SLAM/icp.py (inverse of a finite H times a NaN right-hand side); no golden records it."""
    sc = scene(("nan_residual",))
    want, n, info = oracle_step(sc, sc["pose"], 1e-6)
    (before, after, cnt), = gauss_newton(icp, sc, sc["pose"], 1e-6)
    assert cnt == n
    assert np.array_equal(np.isnan(after), np.isnan(want)) and np.array_equal(after[3], want[3])


def test_host_solve_agrees_with_device_solve_on_rank3(icp):
    torch, M = icp
    sc = scene(("rank3",))
    v0, v1, n0, n1 = maps_on_gpu(torch, sc)
    host = M.ICP(max_iter=1, damping=0.0, distance_threshold=sc["thr_d"], normal_threshold=20)
    assert float(np.float32(host.normal_threshold)) == sc["thr_n"]
    hp, ratio = host.icp(torch.tensor(sc["pose"], device="cuda"), v0, v1, n0, n1, torch.tensor(sc["K"]))
    (before, after, cnt), = gauss_newton(icp, sc, sc["pose"], 0.0, maps=[v0, v1, n0, n1])
    assert_pose_close(hp.cpu().numpy(), after.astype(np.float64), "host solve vs device solve, rank 3")
    assert abs(float(ratio) - cnt / v0.shape[0] / v0.shape[1]) < 1e-6
