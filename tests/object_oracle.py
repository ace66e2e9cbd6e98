"""Test-side oracle of the object stage (include/dqo_raster.h: dqo_objmap_frame / dqo_objmap_optimize / dqo_objmap_mean_iou;
dqo_quadrics.ObjectMap): a numpy restatement of the statements Mapping.mapping runs for a frame with detections
(SLAM/multiprocess/mapper.py:147-165) — detections_filter (quadrics.py:336-386), ObjectsInitialization / Object.__init__ (:429-538),
Occlusions_Check (:926-968), the live MatchObject (Only_IOU = True, :1013-1217), remove_outlier (:2397-2425) — with Ellipse (:148-248),
Ellipsoid.project (:388-408), Calculate_distance (:970-988) and the helpers bbox_area, bboxes_iou, is_cover, bboxes_intersection
(:283-335).  It works on arrays in the layout of the device table, not on Python objects.

store_dtype = float64 reproduces the reference decision for decision (tests/test_object_oracle.py holds it to recorded and live runs of
the reference).  store_dtype = float32 rounds every table field, every stored observation and the two depth numbers of a detection where
the device stores them, and computes in float64 from those: it is what the GPU is held to.

The key rule (csrc/dqo_sample_hash.h, dqo_object_key), all arithmetic modulo 2^32, fmix32 as in that header:
    s   = fmix32(fmix32(seed_lo ^ 0x9e3779b9) ^ seed_hi)
    b   = fmix32(fmix32(s + draw) + frame_id)              draw 8: a depth sample's u, 9: its v, 10: an optimise step's view
    key = fmix32(fmix32(item ^ b) ^ s)                     item = d * 32 + sample (d: the detection's index in the INPUT, before the filter;
                                                           sample 0..29), or uid * 32 + it for the optimise schedule (it 0..19)
    u = int(b0) + key_u mod (int(b2) - int(b0) + 1), v = int(b1) + key_v mod (int(b3) - int(b1) + 1), then clamped to the image (:367-368).
The sum, minimum, maximum and count of a detection's samples run in sample order in float32 (the reference's `sum_d += d` on float32
tensor elements), sum / count is one float32 division.

Two departures from the reference: the table has no orphans — after a covering replacement the per-frame list keeps the
stale projection and category (as the reference's dictionary does) but a later detection matched through it is matched to the ROW; and a
detection reports its row AFTER remove_outlier's compaction, -1 when its object went.

Margins: every comparison of a computed float against a threshold, or of two computed floats, that decides something records
|lhs - rhs| / max(|rhs|, 1).  Not recorded: comparisons on unaltered input data (d > 0 of a depth sample), the continuous clamps
(min(avg, 5), the 0.05..0.2 clamp, clip(cov, 0), d < 0 -> 0), `iou < 0.01 and not valid` (the detection is always valid there), and
`iou > iou_max` between bit-identical values (identical rows give identical results on either side)."""
import numpy as np

FATE_DROPPED, FATE_INVALID, FATE_MATCHED, FATE_NEW, FATE_REPLACED, FATE_UNMATCHED = range(6)
FATES = ("dropped", "invalidated", "matched", "new", "replaced", "unmatched")
HEADER = ("accepted", "matched", "new", "replaced", "removed", "has_new_object", "overflow_obj", "overflow_views")
N_SAMPLES = 30
N_OPT_ITERS = 20
M32 = 0xFFFFFFFF


def _fmix(h):
    h &= M32
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & M32
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & M32
    h ^= h >> 16
    return h


def object_key(seed, draw, frame_id, item):
    seed = int(seed) & (2 ** 64 - 1)
    s = _fmix(_fmix((seed & M32) ^ 0x9E3779B9) ^ (seed >> 32))
    b = _fmix(_fmix(s + draw) + (int(frame_id) & M32))
    return _fmix(_fmix((int(item) & M32) ^ b) ^ s)


def sample_uv(seed, frame_id, d, s, bbox, W, H):
    """Pixel of depth sample s of input detection d (quadrics.py:365-368 with the key rule for random.randint)."""
    lo_u, hi_u, lo_v, hi_v = int(bbox[0]), int(bbox[2]), int(bbox[1]), int(bbox[3])
    u = lo_u + object_key(seed, 8, frame_id, d * 32 + s) % max(hi_u - lo_u + 1, 1)  # (an empty range counts as one value)
    v = lo_v + object_key(seed, 9, frame_id, d * 32 + s) % max(hi_v - lo_v + 1, 1)
    return min(max(u, 0), W - 1), min(max(v, 0), H - 1)


def optimize_schedule(seed, frame_id, uid, nviews):
    """The view of each of the 20 steps (quadrics.py:2264-2266): the key rule modulo the count for it <= 5, the last one afterwards."""
    return [object_key(seed, 10, frame_id, uid * 32 + it) % nviews if it <= N_OPT_ITERS / 4 else nviews - 1 for it in range(N_OPT_ITERS)]


# ---- helpers, quadrics.py:283-335 ------------------------------------------------------------------------------------------------
def bbox_area(bb):
    return (bb[2] - bb[0]) * (bb[3] - bb[1])


def bboxes_intersection(bb1, bb2):
    inter_w = max(min(bb1[2], bb2[2]) - max(bb1[0], bb2[0]), 0)
    inter_h = max(min(bb1[3], bb2[3]) - max(bb1[1], bb2[1]), 0)
    return inter_h * inter_w


def bboxes_iou(bb1, bb2):
    area_inter = bboxes_intersection(bb1, bb2)
    with np.errstate(all="ignore"):
        return np.float64(area_inter) / (bbox_area(bb1) + bbox_area(bb2) - area_inter)


class _Margins:
    def __init__(self):
        self.values = []

    def cmp(self, lhs, rhs):
        with np.errstate(all="ignore"):
            m = abs(float(lhs) - float(rhs)) / max(abs(float(rhs)), 1.0)
        if np.isfinite(m):
            self.values.append(m)

    def lt(self, lhs, rhs):
        self.cmp(lhs, rhs)
        return lhs < rhs

    def gt(self, lhs, rhs):
        self.cmp(lhs, rhs)
        return lhs > rhs

    def le(self, lhs, rhs):
        self.cmp(lhs, rhs)
        return lhs <= rhs


def is_cover(bb1, bb2, mg):
    area_inter = bboxes_intersection(bb1, bb2)
    if bbox_area(bb1) == 0:
        return False
    with np.errstate(all="ignore"):
        return bool(mg.gt(area_inter / bbox_area(bb1), 0.5) and mg.lt(np.float64(area_inter) / bbox_area(bb2), 0.5))


# ---- Ellipse (:148-248), as (centre, squared half axes, bbox, clipped covariance, half axes) -----------------------------------
def detection_ellipse(ell):
    """Ellipse(ell[2:4], ell[4], ell[0:2]) of a json entry [cx, cy, full axis 0, full axis 1, angle] (:262): its ComputeBbox."""
    a0, a1 = 0.5 * float(ell[2]), 0.5 * float(ell[3])
    c, s = np.cos(float(ell[4])), np.sin(float(ell[4]))
    xmax = np.sqrt(a0 ** 2 * c ** 2 + a1 ** 2 * s ** 2)
    ymax = np.sqrt(a0 ** 2 * s ** 2 + a1 ** 2 * c ** 2)
    return np.array([ell[0] - xmax, ell[1] - ymax, ell[0] + xmax, ell[1] + ymax], np.float64)


def ellipsoid_Q(axes, R, center):
    """Ellipsoid.__init__ (:389-400): Q* = [[R A R^T - c c^T, -c], [-c^T, -1]] (already symmetric and normalised)."""
    R = np.asarray(R, np.float64).reshape(3, 3)
    c = np.asarray(center, np.float64)
    Q = np.empty((4, 4))
    Q[:3, :3] = R @ np.diag(np.asarray(axes, np.float64) ** 2) @ R.T - np.outer(c, c)
    Q[:3, 3] = Q[3, :3] = -c
    Q[3, 3] = -1.0
    return 0.5 * (Q + Q.T)


def project(axes, R, center, P):
    """Ellipsoid.project + Ellipse.FromDual + decompose + ComputeBbox + AsGaussian, the 2x2 eigen-decomposition in closed form:
    for [[p, q], [q, r]], m = (p + r) / 2, hd = (p - r) / 2, h = sqrt(hd^2 + q^2), the eigenvalues are m -+ h; with k = hd / h (0 when
    h = 0) the eigenvector of m - h has cos^2 = (1 - k) / 2, so ComputeBbox needs no angle, and V |L| V^T = ((|l1| + |l2|) / 2) I +
    ((|l1| - |l2|) / 2) [[hd, q], [q, -hd]] / h."""
    with np.errstate(all="ignore"):
        C = P @ ellipsoid_Q(axes, R, center) @ P.T
        C = 0.5 * (C + C.T)
        C = C / -C[2, 2]
        mu = -C[:2, 2]
        p, q, r = C[0, 0] + mu[0] * mu[0], C[0, 1] + mu[0] * mu[1], C[1, 1] + mu[1] * mu[1]
        m, hd = 0.5 * (p + r), 0.5 * (p - r)
        h = np.sqrt(hd * hd + q * q)
        a_hi, a_lo = abs(m + h), abs(m - h)
        k, kq = (hd / h, q / h) if h > 0 else (0.0, 0.0)
        xmax = np.sqrt(a_lo * (0.5 * (1 - k)) + a_hi * (0.5 * (1 + k)))
        ymax = np.sqrt(a_lo * (0.5 * (1 + k)) + a_hi * (0.5 * (1 - k)))
        half_sum, half_dif = 0.5 * (a_hi + a_lo), 0.5 * (a_hi - a_lo)
        cov = np.array([[half_sum + half_dif * k, half_dif * kq], [half_dif * kq, half_sum - half_dif * k]])
        return dict(mu=mu, bbox=np.array([mu[0] - xmax, mu[1] - ymax, mu[0] + xmax, mu[1] + ymax]), cov=np.clip(cov, 0, None),
                    axes=np.sqrt(np.array([a_lo, a_hi])))


def calculate_distance(e1, e2, constant_C=10):
    """Calculate_distance (:970-988) with its element-wise square roots."""
    with np.errstate(all="ignore"):
        sigma11 = np.sqrt(e1["cov"])
        sigma121 = np.sqrt(sigma11 @ e2["cov"] @ sigma11)
        dm = e1["mu"] - e2["mu"]
        d = (dm[0] * dm[0] + dm[1] * dm[1]) + np.trace(e1["cov"] + e2["cov"] - 2 * sigma121)
        if d < 0:
            d = 0
        return np.exp(-np.sqrt(d) / constant_C)


# ---- the table ---------------------------------------------------------------------------------------------------------------------
class ObjectTable:
    """The caller-owned state of dqo_objmap_frame: rows [cap_obj], observation slots [cap_obj, cap_views], the state header
    (object count, next uid, whether the first-frame branch has been taken)."""

    def __init__(self, cap_obj, cap_views, store_dtype=np.float64):
        self.cap_obj, self.cap_views, self.dt = cap_obj, cap_views, np.dtype(store_dtype)
        self.axes = np.zeros((cap_obj, 3), self.dt)
        self.R = np.zeros((cap_obj, 9), self.dt)
        self.center = np.zeros((cap_obj, 3), self.dt)
        self.cat = np.zeros(cap_obj, np.int32)
        self.uid = np.zeros(cap_obj, np.int32)
        self.nviews = np.zeros(cap_obj, np.int32)
        self.view_P34 = np.zeros((cap_obj, cap_views, 12), self.dt)
        self.view_bbox = np.zeros((cap_obj, cap_views, 4), self.dt)
        self.state = np.zeros(3, np.int32)

    @property
    def n(self):
        return int(self.state[0])

    def move_row(self, dst, src):
        for a in (self.axes, self.R, self.center, self.cat, self.uid, self.nviews, self.view_P34, self.view_bbox):
            a[dst] = a[src]


def preset_rows(t, rows, K):
    """Rows a sequence starts from, as an earlier optimise call would have left them: dict(axes, R [9], center, cat, bbox, Rt) each, one
    observation; the first-frame branch counts as taken."""
    for i, r in enumerate(rows):
        t.axes[i], t.R[i], t.center[i] = r["axes"], np.asarray(r["R"]).reshape(9), r["center"]
        t.cat[i], t.uid[i], t.nviews[i] = r["cat"], i, 1
        t.view_P34[i, 0] = (np.asarray(K, np.float64) @ np.asarray(r["Rt"], np.float64)[:3]).reshape(12)
        t.view_bbox[i, 0] = r["bbox"]
    t.state[:] = (len(rows), len(rows), 1)


def object_init(bb, depth2, K, Rt):
    """Object.__init__ (:451-482): (axes, R row-major, centre) of a fresh object, in float64."""
    avg_depth, diff_depth = float(depth2[0]), float(depth2[1])
    bb = np.asarray(bb, np.float64)
    u = ((bb[0] + bb[2]) / 2 - K[0, 2]) / K[0, 0]
    v = ((bb[1] + bb[3]) / 2 - K[1, 2]) / K[1, 1]
    cam = np.array([u * avg_depth, v * avg_depth, avg_depth])
    Rcw, tcw = Rt[:3, :3], Rt[:3, 3]
    center_world = Rcw.T @ cam + (-Rcw.T @ tcw)
    zc = cam / np.sqrt(cam[0] * cam[0] + cam[1] * cam[1] + cam[2] * cam[2])
    xc = np.array([zc[2], 0.0, -zc[0]])  # cross((0, 1, 0), zc)
    xc = xc / np.sqrt(xc[0] * xc[0] + xc[1] * xc[1] + xc[2] * xc[2])
    yc = np.cross(zc, xc)
    rot_world = Rcw.T @ np.stack([xc, yc, zc], axis=1)
    axes = np.array([(bb[2] - bb[0]) * avg_depth / K[0, 0] * 0.5, (bb[3] - bb[1]) * avg_depth / K[1, 1] * 0.5, diff_depth * 0.5])
    return axes, rot_world.reshape(9), center_world


def _write_object(t, row, cat, bb, depth2, K, Rt, P):
    axes, R, center = object_init(bb, depth2, K, Rt)
    t.axes[row], t.R[row], t.center[row] = axes, R, center
    t.cat[row], t.uid[row], t.nviews[row] = cat, t.state[1], 1
    t.state[1] += 1
    t.view_P34[row, 0], t.view_bbox[row, 0] = P.reshape(12), bb


def _append_view(t, row, bb, P, hdr):
    if t.nviews[row] >= t.cap_views:
        hdr["overflow_views"] += 1
        return
    t.view_P34[row, t.nviews[row]], t.view_bbox[row, t.nviews[row]] = P.reshape(12), bb
    t.nviews[row] += 1


def _project_row(t, row, P):
    return project(t.axes[row].astype(np.float64), t.R[row].astype(np.float64), t.center[row].astype(np.float64), P)


def depth_statistics(depth, bbox, d, W, H, frame_id, seed, dt):
    """quadrics.py:358-380 for input detection d: (min(mean, 5), clamp(max - min, 0.05, 0.2)), or (0, 0) without a positive sample."""
    F = np.float32
    sum_d, min_d, max_d, count = F(0), F(100.0), F(-1.0), 0
    for s in range(N_SAMPLES):
        u, v = sample_uv(seed, frame_id, d, s, bbox, W, H)
        x = F(depth[v, u])
        if x > 0.0:
            sum_d = F(sum_d + x)
            count += 1
            min_d, max_d = min(min_d, x), max(max_d, x)
    if count == 0:
        return np.zeros(2, dt), 0
    avg = min(float(F(sum_d / F(count))), 5.0)
    dif = min(max(float(F(max_d - min_d)), 0.05), 0.2)
    return np.array([avg, dif]).astype(dt), count


def frame(t, dets, depth, K, Rt, W, H, frame_id, seed):
    """One frame with detections: mapper.py:155-163 on table t (updated in place).  dets: dict(bbox [M,4], ellipse [M,5], cat [M],
    score [M]).  Returns dict(fate, row, depth [M,2], opt_flag [cap_obj], header {name: int}, events (set of str), margins (list))."""
    bbox = np.asarray(dets["bbox"], np.float64).reshape(-1, 4)
    ell = np.asarray(dets["ellipse"], np.float64).reshape(-1, 5)
    cat, score = np.asarray(dets["cat"]).reshape(-1), np.asarray(dets["score"], np.float64).reshape(-1)
    K, Rt = np.asarray(K, np.float64), np.asarray(Rt, np.float64)[:3]
    depth = np.asarray(depth, np.float32)
    M = len(cat)
    mg, ev = _Margins(), set()
    hdr = dict.fromkeys(HEADER, 0)
    fate = np.full(M, FATE_DROPPED, np.int32)
    rows = np.full(M, -1, np.int32)
    depth2 = np.zeros((M, 2), t.dt)
    P = K @ Rt
    Pst = P.astype(t.dt)  # the observation as the table stores it

    # ---- detections_filter, :336-386 ----
    acc = []
    for d in range(M):
        area = bbox_area(bbox[d])
        if mg.lt(score[d], 0.2):
            ev.add("drop_score")
            continue
        if mg.lt(area, 300):
            ev.add("drop_small")
            continue
        if mg.gt(area, 0.5 * H * W):
            ev.add("drop_large")
            continue
        if mg.lt(bboxes_iou(bbox[d], detection_ellipse(ell[d])), 0.2):
            ev.add("drop_ellipse")
            continue
        similar = False
        for j in acc:
            iou = bboxes_iou(bbox[d], bbox[j])
            if cat[d] == cat[j]:
                if mg.gt(iou, 0.3):
                    similar = True
                    ev.add("drop_same_category")
            elif mg.gt(iou, 0.6):
                similar = True
                ev.add("drop_other_category")
        if not similar:
            acc.append(d)
    hdr["accepted"] = len(acc)
    for d in acc:
        depth2[d], count = depth_statistics(depth, bbox[d], d, W, H, frame_id, seed, t.dt)
        if count == 0:
            ev.add("all_samples_zero")
    dd = depth2.astype(np.float64)

    def new_object(d):
        if t.n >= t.cap_obj:
            hdr["overflow_obj"] += 1
            ev.add("overflow_obj")
            return -1
        row = t.n
        _write_object(t, row, cat[d], bbox[d].astype(t.dt), dd[d], K, Rt, Pst)
        t.state[0] += 1
        return row

    opt_flag = np.zeros(t.cap_obj, np.uint8)
    if not t.state[2]:
        # ---- ObjectsInitialization, :514-538 (Map_global is None) ----
        t.state[2] = 1
        ev.add("first_frame")
        for d in acc:
            if dd[d, 0] != 0.0 and mg.gt(dd[d, 0], 0.0) and mg.lt(dd[d, 0], 15.0):  # (an exact 0: no positive sample)
                fate[d], rows[d] = FATE_NEW, new_object(d)
                if dd[d, 0] <= 0.01:
                    ev.add("first_frame_takes_depth_below_0.01")
            else:
                fate[d] = FATE_UNMATCHED
                ev.add("too_shallow" if dd[d, 0] <= 0.0 else "too_deep")
        hdr["has_new_object"] = 1
    else:
        # ---- Occlusions_Check, :926-968: the visible list, in insertion (row) order ----
        n0 = t.n
        proj0 = [_project_row(t, i, P) for i in range(n0)]
        zs = [float(Rt[2] @ np.append(t.center[i].astype(np.float64), 1.0)) for i in range(n0)]
        img_bbox = np.array([0.0, 0.0, W, H])
        vis = []
        for i in range(n0):
            bb_proj = proj0[i]["bbox"]
            if mg.lt(zs[i], 0):
                ev.add("behind_camera")
                continue
            if mg.lt(bboxes_intersection(bb_proj, img_bbox), 0.3 * bbox_area(bb_proj)):
                ev.add("outside_image")
                continue
            vis.append(i)
            for j in vis:
                if j != i and mg.gt(bboxes_iou(proj0[j]["bbox"], bb_proj), 0.8):
                    if mg.lt(zs[i], zs[j]):
                        vis.remove(j)
                        ev.add("hidden_farther_earlier")
                    else:
                        vis.remove(i)
                        ev.add("hidden_farther_later")
                    break
        list_cat = {i: int(t.cat[i]) for i in vis}  # the per-frame list keeps the category and projection it was built with
        contest = {i: None for i in vis}            # (position among the accepted detections, iou) of this frame's holder

        # ---- MatchObject, :1013-1160 ----
        det_obj = {d: False for d in acc}  # det["obj"] is not None
        valid = {d: True for d in acc}
        for order, d in enumerate(acc):
            iou_max, node, replaced = 0.0, -1, False
            bb_det = bbox[d]
            for i in vis:
                bb_proj = proj0[i]["bbox"]
                iou = bboxes_iou(bb_proj, bb_det)
                if list_cat[i] == cat[d] and mg.lt(iou, 0.5):
                    if is_cover(bb_proj, bb_det, mg):
                        _write_object(t, i, cat[d], bbox[d].astype(t.dt), dd[d], K, Rt, Pst)
                        node, iou_max, replaced = i, 1.0, True
                        ev.add("replaced")
                        break
                    elif is_cover(bb_det, bb_proj, mg):
                        valid[d] = False
                        node, iou_max = -1, 0.0
                        ev.add("covered_invalidated")
                        break
                if mg.gt(iou, 0.5) and iou != iou_max:
                    mg.cmp(iou, iou_max)
                if iou > iou_max and iou > 0.5:
                    iou_max, node = iou, i
            if iou_max > 0.5:
                if not replaced:  # a fresh Object holds no contest state
                    if contest[node] is not None:
                        if mg.lt(iou_max, contest[node][1]):
                            ev.add("contest_lost_by_later")
                            continue
                        det_obj[acc[contest[node][0]]] = False
                        ev.add("contest_won_by_later")
                    contest[node] = (order, iou_max)
                else:
                    hdr["replaced"] += 1
                det_obj[d] = True
                rows[d] = node
                fate[d] = FATE_REPLACED if replaced else FATE_MATCHED
                if not replaced:
                    ev.add("matched")
                pr = _project_row(t, node, P)
                if bboxes_iou(pr["bbox"], bb_det) < 0.01 and not valid[d]:
                    continue
                if mg.le(pr["axes"][0], 0.001) or mg.le(pr["axes"][1], 0.001):
                    ev.add("append_gate")
                    continue
                if replaced:
                    ev.add("doubled_observation")
                if t.nviews[node] >= t.cap_views:
                    ev.add("overflow_views")
                _append_view(t, node, bbox[d].astype(t.dt), Pst, hdr)

        # ---- new objects, :1164-1186 ----
        for d in acc:
            if det_obj[d]:
                continue
            rows[d] = -1
            if not valid[d]:
                fate[d] = FATE_INVALID
            elif dd[d, 0] != 0.0 and mg.gt(dd[d, 0], 0.01) and mg.lt(dd[d, 0], 15.0):
                fate[d], rows[d] = FATE_NEW, new_object(d)
                hdr["has_new_object"] = 1
                ev.add("new_object")
            else:
                fate[d] = FATE_UNMATCHED
                ev.add("too_shallow" if dd[d, 0] <= 0.01 else "too_deep")
                if 0.0 < dd[d, 0] <= 0.01:
                    ev.add("later_frame_refuses_depth_below_0.01")

        # ---- remove_outlier, :2397-2425: row j goes when any row i < j of its category is far from it ----
        n1 = t.n
        pr = [_project_row(t, i, P) for i in range(n1)]
        gone = np.zeros(n1, bool)
        for j in range(n1):
            for i in range(j):
                if t.cat[i] == t.cat[j] and mg.lt(calculate_distance(pr[i], pr[j]), 0.1):
                    gone[j] = True
        new_index = np.cumsum(~gone) - 1
        for j in range(n1):
            if not gone[j] and new_index[j] != j:
                t.move_row(new_index[j], j)
                ev.add("rows_shifted")
        t.state[0] = n1 - int(gone.sum())
        hdr["removed"] = int(gone.sum())
        if gone.any():
            ev.add("outlier_removed")
        for d in acc:
            if rows[d] >= 0:
                rows[d] = -1 if gone[rows[d]] else new_index[rows[d]]

    hdr["matched"] = int((fate == FATE_MATCHED).sum())
    hdr["new"] = int((fate == FATE_NEW).sum())
    # the gate of Object_Optimize_only, :2246-2249
    for d in acc:
        if fate[d] in (FATE_MATCHED, FATE_NEW, FATE_REPLACED) and rows[d] >= 0 and t.nviews[rows[d]] >= 2:
            opt_flag[rows[d]] = 1
    return dict(fate=fate, row=rows, depth=depth2, opt_flag=opt_flag, header=hdr, events=ev, margins=mg.values)


def remove_outlier_literal(cats, pr):
    """The loop of :2403-2418 as written, on a list of (category, projection): the surviving original indices."""
    idx = list(range(len(cats)))
    for i in range(len(idx) - 1, -1, -1):
        for j in range(len(idx) - 1, i, -1):
            if cats[idx[i]] == cats[idx[j]] and calculate_distance(pr[idx[i]], pr[idx[j]]) < 0.1:
                idx.pop(j)
    return idx


def mean_iou(t, K=None):
    """record_iou (mapper.py:1512-1531): each row's mean IoU of its projected bbox with its stored observations, over those with
    IoU > 0; 0 with none.  float64 [cap_obj]."""
    out = np.zeros(t.cap_obj)
    for i in range(t.n):
        s, c = 0.0, 0
        for k in range(int(t.nviews[i])):
            pr = _project_row(t, i, t.view_P34[i, k].astype(np.float64).reshape(3, 4))
            iou = bboxes_iou(t.view_bbox[i, k].astype(np.float64), pr["bbox"])
            if iou > 0:
                s, c = s + iou, c + 1
        out[i] = s / c if c else 0.0
    return out
