"""Scripted multi-frame scenes of the object stage, shared by the CPU oracle tests, the golden generator and the GPU tests
(tests/object_oracle.py states what happens to them).  A 160 x 120 frame, at most 8 detections a frame, 6 or 7 frames a sequence, so the table
carries over.  Every input is a float32 value, so the reference (float64 lists), the oracle and the device read the same numbers.

Each sequence is dict(cap_obj, cap_views, seed, frames=[dict(frame_id, K, Rt, depth [H,W] float32, dets)]); dets is
dict(bbox [M,4], ellipse [M,5], cat [M] int32, score [M]) float32.  EVENTS lists what the sequences must cover between them."""
import numpy as np

W, H = 160, 120
K = np.array([[100.0, 0, 80.0], [0, 100.0, 60.0], [0, 0, 1]], np.float32)

EVENTS = ("drop_score", "drop_small", "drop_large", "drop_ellipse", "drop_same_category", "drop_other_category", "all_samples_zero",
          "behind_camera", "outside_image", "hidden_farther_earlier", "hidden_farther_later", "matched", "contest_won_by_later",
          "contest_lost_by_later", "replaced", "doubled_observation", "covered_invalidated", "append_gate", "new_object", "too_shallow",
          "first_frame_takes_depth_below_0.01", "later_frame_refuses_depth_below_0.01",
          "outlier_removed", "rows_shifted", "overflow_obj", "overflow_views", "first_frame")


def _rt(tx=0.0, ty=0.0, tz=0.0, yaw=0.0):
    c, s = np.cos(yaw), np.sin(yaw)
    return np.array([[c, 0, s, tx], [0, 1, 0, ty], [-s, 0, c, tz]], np.float64).astype(np.float32)


def _depth(regions, base=2.0):
    """base + a ramp of x / 128 over 8 columns, then (x0, y0, x1, y1, value) rectangles with the same ramp (value 0: no depth)."""
    ramp = (np.arange(W) % 8 / 128.0).astype(np.float32)[None, :].repeat(H, 0)
    d = np.float32(base) + ramp
    for x0, y0, x1, y1, v in regions:  # (a value below 1 / 64 stays flat: the ramp would swamp it)
        d[y0:y1, x0:x1] = np.float32(v) if v < 1 / 64 else np.float32(v) + ramp[y0:y1, x0:x1]
    return d.astype(np.float32)


def _dets(items):
    """items: (bbox, cat[, score[, ellipse]]); the default ellipse is the one inscribed in the bbox."""
    bbox, ell, cat, score = [], [], [], []
    for it in items:
        b = it[0]
        bbox.append(b)
        cat.append(it[1])
        score.append(it[2] if len(it) > 2 else 0.9)
        ell.append(it[3] if len(it) > 3 else [(b[0] + b[2]) / 2, (b[1] + b[3]) / 2, b[2] - b[0], b[3] - b[1], 0.0])
    return dict(bbox=np.array(bbox, np.float32).reshape(-1, 4), ellipse=np.array(ell, np.float32).reshape(-1, 5),
                cat=np.array(cat, np.int32), score=np.array(score, np.float32))


def _seq(frames, cap_obj=256, cap_views=64, seed=2024, preset=(), cap_det=8):
    return dict(cap_obj=cap_obj, cap_views=cap_views, cap_det=cap_det, seed=seed, preset=list(preset),
                frames=[dict(frame_id=10 * i + 3, K=K, Rt=rt, depth=dp, dets=_dets(items)) for i, (rt, dp, items) in enumerate(frames)])


def filter_and_contests():
    """The six filter drops and a sample-less detection in the first frame; then a plain match, a too-shallow detection, a contest won by
    the later detection, one lost by it, and new objects."""
    zero = [(96, 26, 146, 86, 0)]
    f0 = (_rt(), _depth(zero), [
        ([20, 20, 60, 70], 1),
        ([100, 90, 130, 115], 2, 0.1),                                    # score
        ([5, 5, 15, 15], 3),                                              # small
        ([0, 0, 150, 110], 4),                                            # large
        ([70, 85, 95, 115], 5, 0.9, [140.0, 20.0, 20.0, 20.0, 0.5]),      # the ellipse is elsewhere
        ([22, 22, 62, 72], 1),                                            # same category, IoU > 0.3 with detection 0
        ([21, 21, 61, 71], 6),                                            # other category, IoU > 0.6 with detection 0
        ([100, 30, 140, 80], 7)])                                         # no depth under it
    f1 = (_rt(), _depth(zero), [([21, 20, 61, 70], 1), ([100, 30, 140, 80], 7), ([66, 70, 96, 110], 8)])
    # two detections over row 0 (projected about [20, 20, 60, 70]), of its category and of another one: the later one is the better
    f2 = (_rt(), _depth(zero), [([20, 20, 60, 56], 1), ([20, 30, 60, 70], 9)])
    # ... and the later one is the worse
    f3 = (_rt(tx=0.125), _depth(zero), [([26, 20, 66, 66], 1), ([26, 38, 66, 70], 10), ([66, 70, 96, 110], 8)])
    f4 = (_rt(tx=0.125, yaw=0.03125), _depth(zero), [([24, 20, 64, 70], 1), ([64, 70, 94, 110], 8)])
    f5 = (_rt(tx=0.25, yaw=0.03125), _depth(zero), [([30, 20, 70, 70], 1), ([110, 90, 150, 118], 11)])
    return _seq([f0, f1, f2, f3, f4, f5], seed=7)


def covers_and_outliers():
    """A covering replacement (with its doubled observation), a covered detection, a detection matched through the stale entry of a
    replaced row, and remove_outlier taking a row that is not the last."""
    f0 = (_rt(), _depth([]), [([60, 40, 90, 70], 1), ([110, 20, 140, 50], 2)])
    f1 = (_rt(), _depth([]), [([50, 30, 110, 90], 1)])                                    # covers row 0
    f2 = (_rt(), _depth([]), [([64, 44, 94, 74], 1), ([110, 20, 140, 50], 2)])            # is covered by row 0
    f3 = (_rt(), _depth([]), [([96, 6, 156, 66], 2), ([110, 20, 140, 52], 3)])            # replaces row 1, then matches its stale entry
    # a second object of category 1 forty pixels from the first goes at once, and the row after it moves up
    f4 = (_rt(), _depth([]), [([4, 80, 34, 110], 1), ([40, 84, 70, 114], 4), ([50, 30, 110, 90], 1)])
    f5 = (_rt(ty=0.0625), _depth([]), [([50, 36, 110, 96], 1), ([40, 90, 70, 118], 4)])
    return _seq([f0, f1, f2, f3, f4, f5], seed=11)


def occlusions_and_views():
    """Objects at depths 1 and 4 that line up after the camera moves sideways (the farther one is hidden, once the earlier row and once
    the later), then objects mostly outside the image and behind the camera."""
    f0 = (_rt(), _depth([(0, 0, 80, 60, 1.0), (80, 0, 160, 60, 4.0)]), [([20, 15, 50, 45], 1), ([120, 10, 150, 40], 2)])
    f1 = (_rt(), _depth([(0, 0, 80, 60, 4.0), (80, 0, 160, 60, 1.0)], base=2.0), [([35, 15, 65, 45], 3), ([105, 10, 135, 40], 4),
                                                                               ([60, 75, 100, 115], 5)])
    # tx = 0.2: depth 1 moves 20 px, depth 4 moves 5 px: rows 0 and 2 meet at [40, 70], rows 1 and 3 at [125, 155]
    f2 = (_rt(tx=0.203125), _depth([]), [([70, 75, 110, 115], 5)])
    f3 = (_rt(tx=0.203125), _depth([]), [([70, 75, 110, 115], 5), ([40, 15, 70, 45], 1)])
    f4 = (_rt(tx=1.0), _depth([]), [([110, 75, 150, 115], 5)])
    f5 = (_rt(tz=-3.0), _depth([]), [([20, 70, 60, 110], 6)])
    f6 = (_rt(tx=0.203125), _depth([]), [([70, 75, 110, 115], 5)])
    return _seq([f0, f1, f2, f3, f4, f5, f6], seed=13)


def overflow():
    """cap_obj = 4 and cap_views = 2: the fifth object and a row's third observation are dropped and counted."""
    a, b, c = ([10, 10, 40, 40], 1), ([60, 10, 90, 40], 2), ([110, 10, 140, 40], 3)
    f0 = (_rt(), _depth([]), [a, b, c])
    f1 = (_rt(), _depth([]), [a, ([10, 70, 40, 100], 4), ([60, 70, 90, 100], 5)])
    f2 = (_rt(), _depth([]), [a, b, ([110, 70, 140, 100], 6)])
    f3 = (_rt(), _depth([]), [a, b, c])
    f4 = (_rt(), _depth([]), [([4, 4, 64, 64], 1), c])   # a covering replacement fills both of the row's slots
    f5 = (_rt(), _depth([]), [([4, 4, 64, 64], 1), b])
    return _seq([f0, f1, f2, f3, f4, f5], cap_obj=4, cap_views=2, seed=17)


def depth_gates():
    """The two depth gates: a mean depth of 1 / 128 makes an object in the first frame (0 < depth) and none in a later one (0.01 < depth)."""
    thin = [(100, 20, 150, 70, 1 / 128), (100, 75, 150, 118, 1 / 128)]
    a, b = ([20, 20, 60, 70], 1), ([20, 76, 56, 112], 4)
    f0 = (_rt(), _depth(thin), [a, ([105, 25, 145, 65], 2)])
    f1 = (_rt(), _depth(thin), [a, ([105, 80, 145, 112], 3)])
    f2 = (_rt(), _depth(thin), [a, b])
    f3 = (_rt(ty=0.0625), _depth(thin), [([20, 23, 60, 73], 1), ([20, 79, 56, 115], 4)])
    f4 = (_rt(), _depth(thin), [a, b, ([105, 80, 145, 112], 3)])
    f5 = (_rt(), _depth(thin), [a, b])
    return _seq([f0, f1, f2, f3, f4, f5], seed=19)


def needle():
    """The append gate: the table starts with a needle (two axes of a micrometre, as an optimise call can leave them) that lies diagonally
    in the image, so its projected bbox is a proper square while one projected axis is below 0.001: a detection matches it and its
    observation is not stored."""
    c = np.float32(np.sqrt(0.5))
    rows = [dict(axes=np.array([0.3, 1e-6, 1e-6], np.float32), R=np.array([[c, -c, 0], [c, c, 0], [0, 0, 1]], np.float32),
                 center=np.array([0.4, 0.2, 2.0], np.float32), cat=1, bbox=np.array([89, 59, 111, 81], np.float32), Rt=_rt()),
            dict(axes=np.array([0.3, 0.4, 0.1], np.float32), R=np.eye(3, dtype=np.float32), center=np.array([-0.8, -0.4, 2.0], np.float32),
                 cat=2, bbox=np.array([25, 20, 55, 60], np.float32), Rt=_rt())]
    n, o = ([89, 59, 111, 81], 1), ([25, 20, 55, 60], 2)
    frames = [(_rt(), _depth([]), [n, o]), (_rt(), _depth([]), [n]), (_rt(ty=0.0625), _depth([]), [([89, 62, 111, 84], 1), ([25, 23, 55, 63], 2)]),
              (_rt(), _depth([]), [o, n]), (_rt(), _depth([]), [n, ([120, 90, 150, 115], 3)]), (_rt(), _depth([]), [n, o])]
    return _seq(frames, seed=23, preset=rows)


def many_detections():
    """More detections than the 32 a single round of the depth fetch covers: 40 accepted ones on a grid, new in the first frame, matched
    in the second, and so on.  Not one of SEQUENCES (whose frames hold at most 8 detections)."""
    cells = [([20 * (i % 8) + 1, 20 * (i // 8) + 1, 20 * (i % 8) + 19, 20 * (i // 8) + 19], i + 1) for i in range(48)]
    f0 = (_rt(), _depth([]), cells[:40])
    f1 = (_rt(), _depth([]), cells[:40])
    f2 = (_rt(), _depth([(0, 0, 160, 40, 3.0)]), cells[8:48])
    return _seq([f0, f1, f2], seed=29, cap_det=64)


SEQUENCES = dict(filter_and_contests=filter_and_contests, covers_and_outliers=covers_and_outliers,
                 occlusions_and_views=occlusions_and_views, overflow=overflow, depth_gates=depth_gates,
                 needle=needle)
WIDE = dict(many_detections=many_detections)  # beyond the scenes' sizes: held to the reference and run on the GPU, not part of the event cover
ALL = dict(SEQUENCES, **WIDE)


def run_oracle(seq, store_dtype, cap_obj=None, cap_views=None):
    """The oracle over one sequence: (table, [frame outputs], [table snapshot after each frame])."""
    import copy
    import object_oracle as O
    t = O.ObjectTable(cap_obj or seq["cap_obj"], cap_views or seq["cap_views"], store_dtype)
    O.preset_rows(t, seq["preset"], K) if seq["preset"] else None
    outs, snaps = [], []
    for f in seq["frames"]:
        outs.append(O.frame(t, f["dets"], f["depth"], f["K"], f["Rt"], W, H, f["frame_id"], seq["seed"]))
        snaps.append(copy.deepcopy(t))
    return t, outs, snaps
