"""numpy restatement of csrc/map_traj.hip — dqo_traj_append, dqo_track_world_maps, dqo_eval_ate — one rounding per statement, in the
kernels' order of operations (the file is compiled with -ffp-contract=off): float64, and float32 for the maps.
tests/test_traj_oracle.py holds it to values recorded from the reference's own functions (tests/golden/traj_golden.npz);
tests/test_gpu_traj.py holds the kernels to it."""
import numpy as np

TESTED, KEYFRAME, LISTED = 1, 2, 4  # DQO_TRAJ_* (include/dqo_raster.h)
f32, f64 = np.float32, np.float64


def matmul4(A, B, dtype=f64):
    """[4,4] @ [4,4] with every entry ((a0 b0 + a1 b1) + a2 b2) + a3 b3 in `dtype`."""
    A, B = np.asarray(A, dtype), np.asarray(B, dtype)
    out = np.empty((4, 4), dtype)
    for r in range(4):
        for c in range(4):
            out[r, c] = ((A[r, 0] * B[0, c] + A[r, 1] * B[1, c]) + A[r, 2] * B[2, c]) + A[r, 3] * B[3, c]
    return out


def invert_affine(P):
    """(W [3,3], T [3]) of the affine pose's inverse by the cofactors of its 3x3 block, in double (traj_invert_affine)."""
    P = np.asarray(P, f64)
    (r00, r01, r02), (r10, r11, r12), (r20, r21, r22) = P[0, :3], P[1, :3], P[2, :3]
    c00, c01, c02 = r11 * r22 - r12 * r21, r12 * r20 - r10 * r22, r10 * r21 - r11 * r20
    c10, c11, c12 = r02 * r21 - r01 * r22, r00 * r22 - r02 * r20, r01 * r20 - r00 * r21
    c20, c21, c22 = r01 * r12 - r02 * r11, r02 * r10 - r00 * r12, r00 * r11 - r01 * r10
    det = (r00 * c00 + r01 * c01) + r02 * c02
    W = np.array([[c00 / det, c10 / det, c20 / det], [c01 / det, c11 / det, c21 / det], [c02 / det, c12 / det, c22 / det]], f64)
    t = P[:3, 3]
    T = np.array([-((W[a, 0] * t[0] + W[a, 1] * t[1]) + W[a, 2] * t[2]) for a in range(3)], f64)
    return W, T


def camera(P, projection=None):
    """dict(c2w [4,4] f32, viewmatrix [4,4] f32 (= w2c transposed), projmatrix [4,4] f32 or None, campos [3] f32) of the world pose P."""
    P = np.asarray(P, f64)
    W, T = invert_affine(P)
    V = np.zeros((4, 4), f64)
    V[:3, :3], V[3, :3], V[3, 3] = W.T, T, 1.0
    return dict(c2w=P.astype(f32), viewmatrix=V.astype(f32), campos=P[:3, 3].astype(f32),
                projmatrix=None if projection is None else matmul4(V, np.asarray(projection, f32).astype(f64)).astype(f32))


def keyframe_metric(Pk, Pc):
    """(theta in degrees, l2) of check_keyframe between the keyframe pose Pk and the current pose Pc (both c2w, double)."""
    Wk, Tk = invert_affine(Pk)
    Wc, Tc = invert_affine(Pc)
    d = [(Wk[0, j] * Wc[0, j] + Wk[1, j] * Wc[1, j]) + Wk[2, j] * Wc[2, j] for j in range(3)]
    cs = (((d[0] + d[1]) + d[2]) - 1.0) / 2.0
    with np.errstate(invalid="ignore"):
        theta = np.arccos(cs) * (180.0 / 3.14159265358979323846)
    e = Tk - Tc
    return f64(theta), f64(np.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]))


class Trajectory:
    """The state dqo_traj_append keeps, appended to one row at a time."""

    def __init__(self, cap, projection=None, gaussian_update_frame=0, theta_thres=0.0, trans_thres=0.0, init_pose=None):
        self.cap, self.projection, self.guf, self.theta_thres, self.trans_thres = cap, projection, gaussian_update_frame, theta_thres, trans_thres
        self.init_pose = init_pose
        self.pose, self.pose_gt = np.zeros((cap, 4, 4), f64), np.zeros((cap, 4, 4), f64)
        self.flags, self.kf_metric = np.zeros((cap,), np.int32), np.zeros((cap, 2), f64)
        self.count, self.last_keyframe, self.overflow = 0, -1, 0
        self.cam = None

    def append(self, pose, relative=True, pose_gt=None):
        i = self.count
        if i >= self.cap:
            self.overflow = 1
            return
        if not relative:
            P = np.asarray(pose, f64).copy()
        elif i == 0:
            P = np.eye(4) if self.init_pose is None else np.asarray(self.init_pose, f64).copy()
        else:
            P = matmul4(self.pose[i - 1], np.asarray(pose, f32).astype(f64))
        self.pose[i] = P
        if pose_gt is not None:
            self.pose_gt[i] = pose_gt
        self.cam = camera(P, self.projection)
        flag, theta, l2 = 0, 0.0, 0.0
        if self.guf > 0 and (i == 0 or (i + 1) % self.guf == 0):
            flag = TESTED
            if self.last_keyframe < 0:
                flag |= LISTED
                self.last_keyframe = i
            else:
                theta, l2 = keyframe_metric(self.pose[self.last_keyframe], P)
                if theta > self.theta_thres or l2 > self.trans_thres:
                    flag |= KEYFRAME | LISTED
                    self.last_keyframe = i
        self.flags[i], self.kf_metric[i] = flag, (theta, l2)
        self.count = i + 1


def world_maps(vertex_c, normal_c, c2w):
    """(vertex_w, normal_w) in float32: ((r0 x + r1 y) + r2 z) + t per component, the normals without t."""
    M = np.asarray(c2w, f32).reshape(4, 4)
    out = []
    for m, translate in ((vertex_c, True), (normal_c, False)):
        m = np.asarray(m, f32)
        x, y, z = m[..., 0], m[..., 1], m[..., 2]
        comps = []
        for c in range(3):
            v = (M[c, 0] * x + M[c, 1] * y) + M[c, 2] * z
            comps.append(v + M[c, 3] if translate else v)
        out.append(np.stack(comps, -1).astype(f32))
    return out[0], out[1]


def _lane_tree(part):
    """Sum of up to 256 per-thread values [256, q] as the block does it: xor butterfly in each wave of 64, the four waves in order."""
    w = part.reshape(4, 64, -1)
    for off in (32, 16, 8, 4, 2, 1):
        w = w + w[:, np.arange(64) ^ off]
    w = w[:, 0]
    return ((w[0] + w[1]) + w[2]) + w[3]


def _thread_sums(vals):
    """[n, q] values -> [256, q]: thread t adds rows t, t + 256, ... in order."""
    n, q = vals.shape
    pad = (-n) % 256
    v = np.concatenate([vals, np.zeros((pad, q), f64)]).reshape(-1, 256, q)
    acc = np.zeros((256, q), f64)
    for k in range(v.shape[0]):
        acc = acc + v[k]  # (adding the padding's +0.0 changes nothing: x + 0.0 == x, and the sums start at +0.0)
    return acc


def horn_rotation(S):
    """ate_horn_rotation: the rotation from S[a, b] = sum model_a data_b by cyclic Jacobi on Horn's 4x4."""
    (Sxx, Sxy, Sxz), (Syx, Syy, Syz), (Szx, Szy, Szz) = np.asarray(S, f64)
    A = np.array([[(Sxx + Syy) + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx],
                  [Syz - Szy, (Sxx - Syy) - Szz, Sxy + Syx, Szx + Sxz],
                  [Szx - Sxz, Sxy + Syx, (Syy - Sxx) - Szz, Syz + Szy],
                  [Sxy - Syx, Szx + Sxz, Syz + Szy, (Szz - Sxx) - Syy]], f64)
    V = np.eye(4)
    for _ in range(64):
        off = diag = f64(0.0)
        for p in range(4):
            diag += A[p, p] * A[p, p]
            for q in range(p + 1, 4):
                off += A[p, q] * A[p, q]
        if not off > 1e-34 * diag:
            break
        for p in range(3):
            for q in range(p + 1, 4):
                apq = A[p, q]
                if apq == 0.0:
                    continue
                with np.errstate(over="ignore"):  # a tiny apq: theta * theta may be inf, t is then 0 (as in the kernel)
                    theta = (A[q, q] - A[p, p]) / (2.0 * apq)
                    t = (1.0 if theta >= 0.0 else -1.0) / (abs(theta) + np.sqrt(theta * theta + 1.0))
                c = 1.0 / np.sqrt(t * t + 1.0)
                sn = t * c
                for M_ in (A, V):
                    kp, kq = M_[:, p].copy(), M_[:, q].copy()
                    M_[:, p], M_[:, q] = c * kp - sn * kq, sn * kp + c * kq
                    if M_ is A:
                        pk, qk = A[p, :].copy(), A[q, :].copy()
                        A[p, :], A[q, :] = c * pk - sn * qk, sn * pk + c * qk
    m = 0
    for k in range(1, 4):
        if A[k, k] > A[m, m]:
            m = k
    w, x, y, z = V[:, m]
    nrm = np.sqrt(((w * w + x * x) + y * y) + z * z)
    if not nrm > 0.0 or not np.isfinite(nrm):
        w, x, y, z = 1.0, 0.0, 0.0, 0.0
    else:
        w, x, y, z = w / nrm, x / nrm, y / nrm, z / nrm
    return np.array([[((w * w + x * x) - y * y) - z * z, 2.0 * (x * y - w * z), 2.0 * (x * z + w * y)],
                     [2.0 * (x * y + w * z), ((w * w - x * x) + y * y) - z * z, 2.0 * (y * z - w * x)],
                     [2.0 * (x * z - w * y), 2.0 * (y * z + w * x), ((w * w - x * x) - y * y) + z * z]], f64)


def ate_prefix(model, data):
    """(ate in cm, rot [3,3], trans [3]) of one prefix: model = ground truth, data = estimate, [n,3] double."""
    model, data = np.asarray(model, f64), np.asarray(data, f64)
    n = model.shape[0]
    mean = _lane_tree(_thread_sums(np.concatenate([model, data], 1))) / f64(n)
    mz, dz = model - mean[:3], data - mean[3:]
    S = _lane_tree(_thread_sums((mz[:, :, None] * dz[:, None, :]).reshape(n, 9))).reshape(3, 3)
    R = horn_rotation(S)
    e = np.stack([((R[a, 0] * mz[:, 0] + R[a, 1] * mz[:, 1]) + R[a, 2] * mz[:, 2]) - dz[:, a] for a in range(3)], 1)
    q = (0.0 + e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
    total = _lane_tree(_thread_sums(q[:, None]))[0]
    trans = np.array([mean[3 + a] - ((R[a, 0] * mean[0] + R[a, 1] * mean[1]) + R[a, 2] * mean[2]) for a in range(3)])
    return np.sqrt(total / f64(n)) * 100.0, R, trans


def ate_curve(model, data):
    """(ate [N], fit [12]) of dqo_eval_ate."""
    N = len(model)
    out = np.empty((N,), f64)
    for i in range(1, N + 1):
        out[i - 1], R, t = ate_prefix(model[:i], data[:i])
    return out, np.concatenate([R.reshape(-1), t])
