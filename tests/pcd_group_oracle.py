"""Oracle of the per-object geometry evaluation (dqo_nn1_grouped, dqo_eval_pcd_grouped): tests/pcd_oracle.py applied per object.

nn1_grouped_oracle       po.nn1_oracle on each group's subsets (as its keep masks), scattered back into the queries' rows.
eval_pcd_objects_oracle  po.eval_pcd_oracle per object, from cKDTree's float64 distances between the object's two subsets.
objects_case             the case "objects" of the tests, and the premises of the GPU bars on it (objects_premises).

A group id in [0, 64) is a row's object; any other value means the row has none and takes no part on either side.
"""
import numpy as np
from scipy.spatial import cKDTree

import pcd_oracle as po

OBJECTS = 64


def groups_of(*ids):
    """The object ids present in every one of the id arrays, ascending."""
    present = None
    for a in ids:
        a = np.asarray(a)
        s = set(int(g) for g in np.unique(a) if 0 <= g < OBJECTS)
        present = s if present is None else present & s
    return sorted(present)


def nn1_grouped_oracle(q, q_group, r, r_group, xforms=(None, None)):
    """(dist2 float32 [Q], idx int32 [Q], d64 float64 [Q]): what dqo_nn1_grouped returns — for every group g the rows of
    po.nn1_oracle(q, r, keeps=(q_group == g, r_group == g)) at the queries of g; FLT_MAX / -1 / inf for a query without a group or whose
    group has no reference."""
    q_group, r_group = np.asarray(q_group), np.asarray(r_group)
    Q = np.asarray(q).shape[0]
    dist2, idx, d64 = np.full((Q,), po.FLT_MAX, np.float32), np.full((Q,), -1, np.int32), np.full((Q,), np.inf)
    for g in groups_of(q_group):
        qk = q_group == g
        d, i, dd = po.nn1_oracle(q, r, (qk, r_group == g), xforms)
        dist2[qk], idx[qk], d64[qk] = d[qk], i[qk], dd[qk]
    return dist2, idx, d64


def eval_pcd_objects_oracle(gt, gt_object, rec, rec_object, dist_thres=(0.01,), transform=None):
    """{object id: (results, counts, rec rows, gt rows, d_rec, d_gt)} for the objects with rows on both sides: po.eval_pcd_oracle of cKDTree's float64
    distances between the object's reconstructed rows (under `transform`, dqo_nn1's float32 rule) and its ground-truth rows."""
    gt, rec = np.asarray(gt, np.float32), po.transform_f32(rec, transform)
    gt_object, rec_object = np.asarray(gt_object), np.asarray(rec_object)
    out = {}
    for g in groups_of(gt_object, rec_object):
        a, b = gt[gt_object == g], rec[rec_object == g]
        d_rec, d_gt = po.kdtree_distances(a, b)
        out[g] = po.eval_pcd_oracle(d_rec, d_gt, dist_thres) + (b.shape[0], a.shape[0], d_rec, d_gt)
    return out


def _box_faces(rng, n, lo, hi):
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    p = lo + rng.uniform(0, 1, (n, 3)) * (hi - lo)
    axis, side = rng.integers(0, 3, n), rng.integers(0, 2, n)
    p[np.arange(n), axis] = np.where(side == 1, hi[axis], lo[axis])
    return p


OBJECTS_THRES = (0.005, 0.01)
OBJECTS_SEED = 53  # (scanned on the CPU: the first seeds leave a distance within 1e-4 relative of a threshold; test_pcd_group_oracle.py asserts the premises)
# a book lying on the table, a cup standing on it, a laptop whose box cuts the book's, and a mug the map never saw
OBJECTS_BOXES = {5: ((0.00, 0.00, 0.00), (0.30, 0.20, 0.04)), 0: ((0.05, 0.06, 0.04), (0.13, 0.14, 0.14)),
                 63: ((0.22, -0.05, 0.01), (0.57, 0.20, 0.04)), 7: ((0.36, 0.22, 0.00), (0.44, 0.30, 0.10))}


def objects_case(seed=OBJECTS_SEED):
    """The case "objects": (gt [9000,3], gt_object [9000], rec [9000,3], rec_object [9000]), float32 / int32, both sets shuffled.
    Ground truth: 2250 points on the faces of each of the four boxes (ids 0, 5, 63 and 7).  Reconstruction: ids 0, 5 and 63 with 2333,
    2333 and 2334 points on the faces plus N(0, 0.004), and 2000 background rows (id -1) spread through the same volume; object 7 has
    no reconstructed row."""
    rng = np.random.default_rng(seed)
    gt = np.concatenate([_box_faces(rng, 2250, *OBJECTS_BOXES[g]) for g in (0, 5, 63, 7)])
    gt_object = np.repeat(np.int32([0, 5, 63, 7]), 2250)
    counts = {0: 2333, 5: 2333, 63: 2334}
    rec = np.concatenate([_box_faces(rng, n, *OBJECTS_BOXES[g]) + rng.normal(0, 0.004, (n, 3)) for g, n in counts.items()]
                         + [rng.uniform(0, 1, (2000, 3)) * np.array([0.62, 0.40, 0.16]) + np.array([-0.02, -0.07, -0.01])])
    rec_object = np.concatenate([np.full((n,), g, np.int32) for g, n in counts.items()] + [np.full((2000,), -1, np.int32)])
    a, b = rng.permutation(9000), rng.permutation(9000)
    return gt[a].astype(np.float32), gt_object[a], rec[b].astype(np.float32), rec_object[b]


def objects_premises(gt, gt_object, rec, rec_object, thres=OBJECTS_THRES, transform=None):
    """The premises of the GPU bars on a grouped case, as a dict of figures (the tests assert them):
        margin      the smallest |d - th| / th over every object, direction and threshold (the bar: above 1e-4, "counts exactly")
        decisive    every object and direction has a threshold whose count lies strictly between 0 and the row count
        foreign     {object: (rec queries, gt queries) whose nearest neighbour REGARDLESS of group belongs to another group or to none}"""
    res = eval_pcd_objects_oracle(gt, gt_object, rec, rec_object, thres, transform)
    margin, decisive = np.inf, True
    for g, (_, counts, n_rec, n_gt, d_rec, d_gt) in res.items():
        for t, th in enumerate(thres):
            margin = min(margin, float((np.abs(d_rec - th) / th).min()), float((np.abs(d_gt - th) / th).min()))
        decisive = decisive and any(0 < c[0] < n_rec for c in counts) and any(0 < c[1] < n_gt for c in counts)
    moved = po.transform_f32(rec, transform)
    near_gt = np.asarray(gt_object)[cKDTree(np.asarray(gt, np.float64)).query(moved.astype(np.float64))[1]]
    near_rec = np.asarray(rec_object)[cKDTree(moved.astype(np.float64)).query(np.asarray(gt, np.float64))[1]]
    foreign = {g: (int(((np.asarray(rec_object) == g) & (near_gt != g)).sum()), int(((np.asarray(gt_object) == g) & (near_rec != g)).sum()))
               for g in res}
    return dict(margin=margin, decisive=decisive, foreign=foreign)


TWO_GROUPS_THRES = (0.03,)


def two_groups_case(seed=32):
    """Two interleaved objects, uniform in the unit cube: rec = 70 001 rows of object 3 and 66 000 of object 40, gt = 135 001 rows of
    object 3 and 66 000 of object 40, both shuffled — 133 and 197 blocks of 1 024 sorted rows, and object 3's ground truth alone spans
    132 of them: more than the 128 partials the reduction's last block stages at a time."""
    rng = np.random.default_rng(seed)
    rec, gt = rng.uniform(0, 1, (136001, 3)).astype(np.float32), rng.uniform(0, 1, (201001, 3)).astype(np.float32)
    rec_object = np.where(np.arange(136001) < 70001, 3, 40).astype(np.int32)
    gt_object = np.where(np.arange(201001) < 135001, 3, 40).astype(np.int32)
    rng.shuffle(rec_object), rng.shuffle(gt_object)
    return gt, gt_object, rec, rec_object


OBJECTS_XFORM = np.array([[0.8, -0.6, 0.0, 0.25], [0.6, 0.8, 0.0, -0.5], [0.0, 0.0, 1.0, 0.125]], np.float32)


def objects_stored_case(seed=OBJECTS_SEED):
    """The case "objects" with the reconstruction stored in another frame: OBJECTS_XFORM moves it back onto the ground truth (up to the
    float32 rounding of the two motions, so its premises are asserted on their own)."""
    gt, gt_object, rec, rec_object = objects_case(seed)
    R3, t3 = OBJECTS_XFORM[:, :3].astype(np.float64), OBJECTS_XFORM[:, 3].astype(np.float64)
    stored = ((rec.astype(np.float64) - t3) @ R3).astype(np.float32)  # (R orthonormal: its inverse is its transpose)
    return gt, gt_object, stored, rec_object
