"""Seeded numpy inputs for the ICP kernels (csrc/icp.hip) at the places where they can go wrong: image sizes around the block and the
launch cap, pixels that sit exactly on every comparison, and normal equations of every rank the device-side solve branches on.

A scene is a dict: v0, v1, n0, n1 [H, W, 3] fp32, pose [4, 4] fp32, K [3, 3] fp32, thr_d, thr_n (floats that are fp32 values).
`check_*` assert, with the oracle on the CPU, that a scene really contains what it is built for."""
import numpy as np

import icp_oracle as O

f32 = np.float32
THR_D = 0.2
THR_N = float(f32(np.cos(np.deg2rad(20))))

# 3x85 = 255 and 16x16 = 256 pixels straddle one block of 256; 513x512 = 262656 is the first such size above the 1024 x 256 = 262144
# threads of the capped launch, so the grid-stride loop takes a second trip
LAUNCH_CAP = 1024 * 256
SWEEP_SIZES = [(2, 2), (2, 129), (3, 85), (16, 16), (17, 23), (513, 512)]


def sweep_pose():
    """Rotation about all three axes (z, then y, then x) and a translation."""
    ax, ay, az = 0.004, -0.007, 0.005
    cx_, sx, cy_, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    Rx = np.array([[1, 0, 0], [0, cx_, -sx], [0, sx, cx_]])
    Ry = np.array([[cy_, 0, sy], [0, 1, 0], [-sy, 0, cy_]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    pose = np.eye(4)
    pose[:3, :3] = Rx @ Ry @ Rz
    pose[:3, 3] = [0.011, -0.004, -0.009]  # moves the image up: the last row stays in view
    return pose.astype(f32)


def sweep_scene(H, W):
    """A smooth depth surface with 5 % holes, seen twice a small motion apart, and intrinsics with non-round values."""
    rng = np.random.default_rng(1000 * H + W)
    K = np.array([[0.93 * W + 0.371, 0, (W - 1) / 2.0 + 0.23], [0, 0.91 * W + 0.113, (H - 1) / 2.0 - 0.31], [0, 0, 1]], f32)
    jj, ii = np.meshgrid(np.arange(W), np.arange(H))
    sw, sh = max(W, 8) / 3.1, max(H, 8) / 2.3
    # an axis of 2 or 3 pixels has (next to) no interior: there frame 0's points are drawn in by 0.4 pixel from both ends, so that
    # some of them project strictly inside
    xs = jj if W > 3 else 0.4 + jj * (W - 1.8) / (W - 1)
    ys = ii if H > 3 else 0.4 + ii * (H - 1.8) / (H - 1)

    def maps(shift):
        z = (2.0 + 0.3 * np.sin((jj + shift) / sw) + 0.2 * np.cos(ii / sh)).astype(f32)
        z[rng.uniform(size=(H, W)) < 0.05] = 0
        v = np.stack([(xs - K[0, 2]) / K[0, 0] * z, (ys - K[1, 2]) / K[1, 1] * z, z], -1).astype(f32)
        n = np.stack([-np.gradient(z, axis=1) * K[0, 0] / np.maximum(z, 1e-3), -np.gradient(z, axis=0) * K[1, 1] / np.maximum(z, 1e-3),
                      np.ones_like(z)], -1)
        return v, (-(n / np.linalg.norm(n, axis=-1, keepdims=True))).astype(f32)

    (v0, n0), (v1, n1) = maps(0.0), maps(0.8)
    return dict(v0=v0, v1=v1, n0=n0, n1=n1, pose=sweep_pose(), K=K, thr_d=THR_D, thr_n=THR_N)


def trace(sc, k_scale=1.0, pose=None):
    return O.trace_pixels(sc["v0"], sc["v1"], sc["n0"], sc["n1"], sc["pose"] if pose is None else pose, *O.intrinsics(sc["K"], k_scale),
                           sc["thr_d"], sc["thr_n"])


def check_sweep(sc):
    """The scene exercises the sums: some pixels count, some do not."""
    ok = trace(sc)["ok"]
    assert 0 < ok.sum() < ok.size or ok.size == 4 and ok.sum() > 0, (ok.sum(), ok.size)
    # above the launch cap, pixels of the grid-stride loop's second trip count, and so do pixels of its first
    assert ok.size <= LAUNCH_CAP or ok.reshape(-1)[LAUNCH_CAP:].sum() > 100 and ok.reshape(-1)[:LAUNCH_CAP].sum() > 100


# ---- the edge scene: a fronto-parallel plane on which every per-pixel quantity is exact ------------------------------------------------
EDGE_H, EDGE_W = 9, 11
EDGE_TX = (0.25, -0.25, 0.125, -0.125)
EDGE_THR_D = 0.25
# frame-0 pixels (row, column) that carry one special each; columns 3 and 6 are in view for every tx and their associations never
# meet in frame 1, the rows keep them apart
EDGE_PIXELS = dict(dist_at=(1, 3), dist_above=(1, 6), normal_at=(2, 3), normal_above=(2, 6), v0z_zero=(3, 3), v0z_negative=(3, 6),
                   qz_zero=(4, 3), pz_negative=(5, 3), v0_nan=(5, 6), v0z_nan=(6, 3), v0z_inf=(6, 6), q_nan=(7, 3))


def edge_scene(tx, with_nan=True):
    """fx = fy = 8, principal point (5, 4), frame 0 a plane at z = 3 moved by t = (tx, 0, -1) onto z = 2 with the identity rotation, so
    u = j + 4 tx and v = i exactly: tx = +-0.25 puts a column exactly on u = W-1 / u = 0, tx = +-0.125 puts every column on a
    half-integer.  Frame 1 has the same lattice at depth 2 + column / 128, so the residual names the sampled column.  Single pixels
    (EDGE_PIXELS) then sit on each remaining comparison.  with_nan=False leaves out the NaN of frame 1, which turns sums into NaN."""
    H, W = EDGE_H, EDGE_W
    K = np.array([[8, 0, 5], [0, 8, 4], [0, 0, 1]], f32)
    jj, ii = np.meshgrid(np.arange(W), np.arange(H))
    up = np.broadcast_to(np.array([0, 0, 1], f32), (H, W, 3))
    v0 = np.stack([(jj - 5) / 4.0, (ii - 4) / 4.0, np.full((H, W), 3.0)], -1).astype(f32)
    v1 = np.stack([(jj - 5) / 4.0, (ii - 4) / 4.0, 2.0 + jj / 128.0], -1).astype(f32)
    n0, n1 = up.copy(), up.copy()
    pose = np.eye(4, dtype=f32)
    pose[:3, 3] = [tx, 0, -1]
    sc = dict(v0=v0, v1=v1, n0=n0, n1=n1, pose=pose, K=K, thr_d=EDGE_THR_D, thr_n=THR_N)
    t = trace(sc)
    E = EDGE_PIXELS

    def target(px):  # the frame-1 pixel that frame-0 pixel `px` is associated with, and its transformed point
        assert t["ok0"][px], px
        return (t["yi"][px], t["xi"][px]), np.array([t["p"][k][px] for k in range(3)], f32)

    q, p = target(E["dist_at"])
    v1[q] = p - np.array([0, 0, 0.25], f32)            # p - q = (0, 0, 0.25): |p - q| == thr_d, which still counts
    q, p = target(E["dist_above"])
    v1[q] = p - np.array([2.0 ** -13, 0, 0.25], f32)   # 0.0625 + 2^-26 is exact; its root rounds to thr_d + one ulp
    n0[E["normal_at"]] = [0, 0, THR_N]                  # n . m == thr_n: does not count
    n0[E["normal_above"]] = [0, 0, np.nextafter(f32(THR_N), f32(1))]
    v0[E["v0z_zero"]][2] = 0
    v0[E["v0z_negative"]] = -v0[E["v0z_negative"]]
    q, _ = target(E["qz_zero"])
    v1[q][2] = 0
    v0[E["pz_negative"]] = [0.125 - tx, 0, 0.5]         # v0z > 0, pz = -0.5, (u, v) = (3, 4) in view
    v0[E["v0_nan"]][0] = np.nan
    v0[E["v0z_nan"]][2] = np.nan
    v0[E["v0z_inf"]][2] = np.inf
    if with_nan:
        q, _ = target(E["q_nan"])
        v1[q][0] = np.nan                               # qz > 0: the pixel counts and the sums turn NaN, as in the reference
    return sc


def check_edge(sc, tx, with_nan=True):
    """Every kind of edge pixel is really met by the oracle, with the outcome its comparison gives."""
    t = trace(sc)
    E, W = EDGE_PIXELS, EDGE_W
    ok, u, gx = t["ok"], t["u"], t["gx"]
    plain = [j for j in range(W) if ok[7, j]]  # row 7 holds at most the frame-1 NaN, which still counts
    if tx == 0.25:
        assert (u[1:8, W - 2] == W - 1).all() and not t["inview"][1:8, W - 2].any() and plain == list(range(0, 9))
    if tx == -0.25:
        assert (u[1:8, 1] == 0).all() and not t["inview"][1:8, 1].any() and plain == list(range(2, 11))
    if abs(tx) == 0.125:
        half = (gx[7] - np.floor(gx[7]) == 0.5) & t["ok0"][7]
        even = half & (np.floor(gx[7]) % 2 == 0)
        assert even.any() and (half & ~even).any(), gx[7]           # halves that round down and halves that round up
        assert plain == (list(range(0, 10)) if tx > 0 else list(range(1, 11)))
        assert len(set(np.asarray(t["r"][7])[ok[7]].tolist())) > 1    # the residual tells the sampled columns apart
    assert t["dn"][E["dist_at"]] == f32(EDGE_THR_D) and ok[E["dist_at"]]
    assert t["dn"][E["dist_above"]] == np.nextafter(f32(EDGE_THR_D), f32(1)) and t["ok0"][E["dist_above"]] and not ok[E["dist_above"]]
    assert t["ndot"][E["normal_at"]] == f32(THR_N) and t["ok0"][E["normal_at"]] and not ok[E["normal_at"]]
    assert t["ndot"][E["normal_above"]] == np.nextafter(f32(THR_N), f32(1)) and ok[E["normal_above"]]
    assert sc["v0"][E["v0z_zero"]][2] == 0 and not ok[E["v0z_zero"]]
    assert sc["v0"][E["v0z_negative"]][2] < 0 and t["inview"][E["v0z_negative"]] and not ok[E["v0z_negative"]]
    assert t["ok0"][E["qz_zero"]] and t["q"][2][E["qz_zero"]] == 0 and not ok[E["qz_zero"]]
    assert t["ok0"][E["pz_negative"]] and t["p"][2][E["pz_negative"]] < 0 and sc["v0"][E["pz_negative"]][2] > 0
    assert not t["inview"][E["v0_nan"]] and not t["ok0"][E["v0z_nan"]]
    assert sc["v0"][E["v0z_inf"]][2] == np.inf and not ok[E["v0z_inf"]]
    if with_nan:
        assert ok[E["q_nan"]] and t["q"][2][E["q_nan"]] > 0 and np.isnan(t["r"][E["q_nan"]])
        assert np.isnan(O.sums(ok, t["J"], t["r"])[1]).any()
    else:
        assert np.isfinite(t["r"]).all() and np.isfinite(t["J"]).all()


# ---- scenes for the device-side solve -----------------------------------------------------------------------------------------------
def rank3_scene():
    """The 9x11 plane at z = 2 with the principal point off centre at (3, 2), every normal (0, 0, 1), the identity pose and a frame 1
    whose depth grows by 1/64 per column and 1/128 per row: J = (py, -px, 0, 0, 0, 1), so rows and columns 2, 3, 4 of JtJ are exactly zero (rank 3) and
    the rest is coupled through the sums of px and py."""
    H, W = EDGE_H, EDGE_W
    K = np.array([[8, 0, 3], [0, 8, 2], [0, 0, 1]], f32)
    jj, ii = np.meshgrid(np.arange(W), np.arange(H))
    up = np.broadcast_to(np.array([0, 0, 1], f32), (H, W, 3))
    v0 = np.stack([(jj - 3) / 4.0, (ii - 2) / 4.0, np.full((H, W), 2.0)], -1).astype(f32)
    v1 = np.stack([(jj - 3) / 4.0, (ii - 2) / 4.0, 2.0 + jj / 64.0 + ii / 128.0], -1).astype(f32)
    return dict(v0=v0, v1=v1, n0=up.copy(), n1=up.copy(), pose=np.eye(4, dtype=f32), K=K, thr_d=EDGE_THR_D, thr_n=THR_N)


def rank1_scene():
    """Only the pixel on the optical axis has depth, and frame 1 is 0.125 behind it: J = (0, 0, 0, 0, 0, 1), r = -0.125."""
    sc = rank3_scene()
    keep = sc["v0"][2, 3].copy()
    sc["v0"][:] = 0
    sc["v0"][2, 3] = keep
    sc["v1"][2, 3, 2] = 2.125
    return sc


def _lone_valid_pixel(sc):
    """A valid pixel whose frame-1 partner no other in-view pixel with depth is associated with."""
    t = trace(sc)
    W = sc["v0"].shape[1]
    flat = (t["yi"] * W + t["xi"])[t["ok0"]]
    uses = np.bincount(flat, minlength=t["ok"].size)
    for i, j in zip(*np.nonzero(t["ok"])):
        if uses[t["yi"][i, j] * W + t["xi"][i, j]] == 1:
            return (i, j), (t["yi"][i, j], t["xi"][i, j]), np.array([t["p"][k][i, j] for k in range(3)], f32)
    raise AssertionError("no pixel with a partner of its own")


def overflow_scene():
    """The 17x23 sweep scene in which one valid pixel makes JtJ non-finite and leaves JtR finite: its partner in frame 1 lies exactly
    on the transformed point (residual 0) and has a normal of length 2^80, so its J^T J terms exceed fp32 (+-inf after the rounding of
    the sums; with damping 0 the diagonal of H is inf * 0 = NaN).  A NaN cannot get there directly: in a normal it fails the normal
    test, in a vertex it makes JtR NaN as well, and then the reference's pose is NaN too (nan_residual_scene)."""
    sc = sweep_scene(17, 23)
    _, q, p = _lone_valid_pixel(sc)
    sc["v1"][q] = p
    sc["n1"][q] = sc["n1"][q] * f32(2.0 ** 80)
    return sc


def nan_residual_scene():
    """The 17x23 sweep scene with a NaN x coordinate at the frame-1 partner of one valid pixel: it still counts, JtR is NaN."""
    sc = sweep_scene(17, 23)
    _, q, _ = _lone_valid_pixel(sc)
    sc["v1"][q][0] = np.nan
    return sc
