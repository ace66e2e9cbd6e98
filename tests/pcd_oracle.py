"""Oracle of the geometry evaluation (dqo_nn1, dqo_eval_pcd): numpy and scipy only.

nn1_oracle      the exact float32 nearest-neighbour distance the kernel must return bit for bit: scipy.spatial.cKDTree finds the
                k = min(8, R) nearest candidates in float64, the kernel's own float32 expression is evaluated on those candidates and its
                minimum taken.  This is exact as long as the float32 minimiser is among the 8 float64-nearest references: a pair's float32
                and float64 squared distances differ by about 1e-7 relative, so it could only fail with 8 references within 1e-7 relative
                of the nearest one (more than 8 coincident references aside, where every one of them gives the same value).
                tests/test_pcd_oracle.py proves it on its inputs against a blocked brute force.
eval_pcd_oracle the five functions of SLAM/eval.py:190-226 and the dict of :263-281, restated line by line in float64.
"""
import numpy as np
from scipy.spatial import cKDTree

FLT_MAX = np.float32(3.4028234663852886e38)


def transform_f32(p, m):
    """dqo_nn1's *_xform: every output row ((m0 * x + m1 * y) + m2 * z) + m3, one float32 rounding per operation."""
    p = np.asarray(p, np.float32)
    if m is None:
        return p
    m = np.asarray(m, np.float32)[:3]
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return np.stack([((m[r, 0] * x + m[r, 1] * y) + m[r, 2] * z) + m[r, 3] for r in range(3)], axis=1).astype(np.float32)


def dist2_f32(a, b):
    """kbest / scan_sub's expression: dx*dx + dy*dy + dz*dz in float32, left to right.  a, b broadcastable [..., 3]."""
    d = (np.asarray(b, np.float32) - np.asarray(a, np.float32)).astype(np.float32)
    return ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]).astype(np.float32)


def brute_force_f32(q, r, block=256):
    """The definition: the minimum of dist2_f32 over ALL references, in blocks of queries.  [Q] float32."""
    q, r = np.asarray(q, np.float32), np.asarray(r, np.float32)
    out = np.empty((q.shape[0],), np.float32)
    for a in range(0, q.shape[0], block):
        out[a:a + block] = dist2_f32(q[a:a + block, None, :], r[None, :, :]).min(axis=1)
    return out


def nn1_oracle(q, r, keeps=(None, None), xforms=(None, None)):
    """(dist2 float32 [Q], idx int32 [Q], d64 float64 [Q]): what dqo_nn1 returns (idx: one of the admissible answers, in the caller's
    numbering), and cKDTree's own float64 distance.  keeps = (query_keep, ref_keep), xforms = (query_xform, ref_xform); a dropped
    query, or any query without a kept reference: FLT_MAX / -1 (d64: inf)."""
    q, r = transform_f32(q, xforms[0]), transform_f32(r, xforms[1])
    Q, R = q.shape[0], r.shape[0]
    qk = np.ones((Q,), bool) if keeps[0] is None else np.asarray(keeps[0]).astype(bool)
    rk = np.ones((R,), bool) if keeps[1] is None else np.asarray(keeps[1]).astype(bool)
    dist2, idx, d64 = np.full((Q,), FLT_MAX, np.float32), np.full((Q,), -1, np.int32), np.full((Q,), np.inf)
    rows, qi = np.nonzero(rk)[0], np.nonzero(qk)[0]
    if rows.size == 0 or qi.size == 0:
        return dist2, idx, d64
    k = min(8, rows.size)
    dd, cand = cKDTree(r[rows].astype(np.float64)).query(q[qi].astype(np.float64), k=k)
    dd, cand = dd.reshape(qi.size, k), cand.reshape(qi.size, k)
    d32 = dist2_f32(q[qi][:, None, :], r[rows][cand])
    best = d32.argmin(axis=1)
    dist2[qi] = d32[np.arange(qi.size), best]
    idx[qi] = rows[cand[np.arange(qi.size), best]].astype(np.int32)
    d64[qi] = dd[:, 0]
    return dist2, idx, d64


def kdtree_distances(gt, rec):
    """(rec -> gt, gt -> rec) float64 distances, as KDTree(a).query(b) of eval.py:191-192, 198-199 returns them."""
    gt, rec = np.asarray(gt, np.float64), np.asarray(rec, np.float64)
    return cKDTree(gt).query(rec)[0], cKDTree(rec).query(gt)[0]


def eval_pcd_oracle(d_rec_to_gt, d_gt_to_rec, dist_thres=(0.03,)):
    """eval_pcd's numbers from the two distance arrays (float64; metres) — the statements of SLAM/eval.py, in float64:
        completion_ratio  :190-194   np.mean(distances(gt -> rec) < dist_th)
        accuracy_ratio    :197-201   np.mean(distances(rec -> gt) < dist_th)
        accuracy          :204-208   np.mean(distances(rec -> gt))
        completion        :211-215   np.mean(distances(gt -> rec))
        chamfer_distance  :218-226   the two means added
        results           :263-281   P, R = ratio * 100; F1 = 2 P R / (P + R); accuracy, completion * 100 (cm)
    Returns (results dict with the reference's keys plus "chamfer", counts): counts[t] = (rec rows under threshold t, gt rows under it)."""
    a, c = np.asarray(d_rec_to_gt, np.float64), np.asarray(d_gt_to_rec, np.float64)
    results = {"accuracy": np.mean(a) * 100, "completion": np.mean(c) * 100}  # :207, :214, :273-274
    Ps, Rs, Fs, counts = {}, {}, {}, []
    for thre in dist_thres:
        P = np.mean((a < thre).astype(np.float64)) * 100  # :200, :264
        R = np.mean((c < thre).astype(np.float64)) * 100  # :193, :265-268
        with np.errstate(invalid="ignore", divide="ignore"):
            F1 = np.float64(2 * P * R) / np.float64(P + R)  # :269
        Ps["P (< {})".format(thre)], Rs["R (< {})".format(thre)], Fs["F1 (< {})".format(thre)] = P, R, F1  # :270-272
        counts.append((int((a < thre).sum()), int((c < thre).sum())))
    results.update(Ps), results.update(Rs), results.update(Fs)  # :279-281
    results["chamfer"] = np.mean(a) + np.mean(c)  # :225
    return results, counts


def room_case(seed=2):
    """The issue's case "room": gt = 5000 points on the faces of a 4 x 3 x 2.5 m box; rec = 4000 such points + N(0, 0.01) noise, the
    first 300 of them shifted by 0.5 m as a floating cluster.  float32 [5000,3], [4000,3]."""
    rng = np.random.default_rng(seed)
    size = np.array([4.0, 3.0, 2.5])

    def faces(n):
        p = rng.uniform(0, 1, (n, 3)) * size
        axis, side = rng.integers(0, 3, n), rng.integers(0, 2, n)
        p[np.arange(n), axis] = side * size[axis]
        return p

    gt = faces(5000)
    rec = faces(4000) + rng.normal(0, 0.01, (4000, 3))
    rec[:300] += 0.5
    return gt.astype(np.float32), rec.astype(np.float32)
