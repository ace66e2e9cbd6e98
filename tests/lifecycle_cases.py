"""Hand-made inputs of the map-maintenance step for tests/test_lifecycle_oracle.py (CPU: the oracle on them, and that every case keeps
its distance from the float thresholds) and tests/test_gpu_lifecycle.py (GPU: the kernels against the oracle, exactly).  numpy / torch on
the CPU only; every case is a pure function of its seed."""
import numpy as np
import torch

H, W = 36, 50  # partial 16 x 16 tiles; H * W = 1800 is no multiple of 256
THRESHOLDS = dict(stable_confidence_thres=20.0, unstable_time_window=30, add_color_thres=0.1, add_depth_thres=0.1)
PARK = np.array([3.0, -2.0, -1.0e4], np.float32)


def make_case(seed, n_alive=600, n_spare=200, tick=100, delete_thresh=10, window=30, stable_outlier=False):
    """dict(state, gt_color, gt_depth, render_color, render_depth, depth_index, color_index, tick, kw, named): a map of n_alive
    Gaussians and n_spare spare rows (ten of them scattered among the live rows, the rest at the tail) and a synthetic frame whose index
    maps name: one row from many pixels, row 0, the last live row, -1, spare rows, the last row, values outside [0, P).  `named`: rows
    with a scripted fate (when the map has at least 100 Gaussians)."""
    rng = np.random.default_rng(seed)
    P = n_alive + n_spare
    thres = THRESHOLDS["stable_confidence_thres"]
    alive = np.zeros(P, np.uint8)
    scattered = min(10, n_spare) if n_alive >= 100 else 0
    live_rows = np.arange(n_alive + scattered)
    if scattered:
        live_rows = np.delete(live_rows, rng.choice(np.arange(1, n_alive + scattered - 1), scattered, replace=False))
    alive[live_rows] = 1
    spare_rows = np.flatnonzero(alive == 0)
    radius = rng.uniform(0.015, 0.03, P).astype(np.float32)
    stable = (rng.random(P) < 0.5).astype(np.uint8)
    confidence = rng.integers(0, int(thres) - 1, P).astype(np.float32)
    add_tick = (tick - rng.integers(0, window - 1, P)).astype(np.int32)
    dcount = rng.integers(0, delete_thresh - 1, P).astype(np.int32)
    ccount = rng.integers(0, delete_thresh - 1, P).astype(np.int32)
    row_flags = rng.integers(0, 2, P).astype(np.uint8)
    named = {}
    if n_alive >= 100:
        pool = list(rng.permutation(live_rows[1:-1]))
        take = lambda n: np.array([pool.pop() for _ in range(n)])
        un = lambda rows: stable.__setitem__(rows, 0)
        st = lambda rows: stable.__setitem__(rows, 1)
        named["promote"], named["at_thres"] = take(8), take(8)      # confidence thres + 1 / exactly thres
        un(named["promote"]), un(named["at_thres"])
        confidence[named["promote"]], confidence[named["at_thres"]] = thres + 1, thres
        named["window"], named["window_plus_1"] = take(5), take(5)  # tick - add_tick == window / window + 1
        un(named["window"]), un(named["window_plus_1"])
        add_tick[named["window"]], add_tick[named["window_plus_1"]] = tick - window, tick - window - 1
        named["oversized"] = take(3)
        un(named["oversized"])
        radius[named["oversized"]] = 1.0
        for k in ("depth_strike", "color_strike", "both_strikes", "unstable_struck", "promoted_and_released", "many_pixels"):
            named[k] = take(1)
        st(named["depth_strike"]), st(named["color_strike"]), st(named["both_strikes"]), st(named["many_pixels"])
        un(named["unstable_struck"]), un(named["promoted_and_released"])
        dcount[named["depth_strike"]] = dcount[named["both_strikes"]] = delete_thresh - 1
        ccount[named["color_strike"]] = ccount[named["both_strikes"]] = delete_thresh - 1
        ccount[named["unstable_struck"]] = dcount[named["unstable_struck"]] = delete_thresh - 1  # (a released row keeps its counters)
        confidence[named["unstable_struck"]] = 3.0
        ccount[named["promoted_and_released"]], confidence[named["promoted_and_released"]] = delete_thresh - 1, thres + 1
        dcount[named["promoted_and_released"]] = 0
        if stable_outlier:  # 30 x the stable cloud's mean radius; the unstable cloud's mean does not see it
            named["stable_outlier"] = take(1)
            st(named["stable_outlier"])
            radius[named["stable_outlier"]] = 30 * 0.0225
    elif n_alive == 1:
        stable[0], confidence[0] = 0, thres + 1
    confidence[stable == 1] = np.minimum(confidence[stable == 1], thres)
    xyz = rng.normal(size=(P, 3)).astype(np.float32)
    opacity_raw = rng.normal(size=(P, 1)).astype(np.float32)
    scaling_raw = np.log(radius[:, None] * np.array([1.0, 1.0, 0.1], np.float32)).astype(np.float32)
    xyz[spare_rows], opacity_raw[spare_rows], scaling_raw[spare_rows], row_flags[spare_rows] = PARK, -10.0, -10.0, 3
    for a in (stable, confidence, add_tick, dcount, ccount):
        a[spare_rows] = 0
    state = dict(xyz=xyz, opacity_raw=opacity_raw, scaling_raw=scaling_raw, confidence=confidence, alive=alive, row_flags=row_flags,
                 stable=stable, add_tick=add_tick, depth_error_counter=dcount, color_error_counter=ccount)

    # the frame: errors are far from the 0.2 the step compares them with (at most 0.05 / 0.03, or at least 0.4 / 0.45)
    n = H * W
    gt_depth = rng.uniform(1.5, 2.5, n).astype(np.float32)
    dclass = rng.choice(3, n, p=[0.85, 0.08, 0.07])  # close | a strike | the render lies BEHIND the target
    cclass = rng.choice(2, n, p=[0.92, 0.08])
    depth_index = rng.integers(0, P, n).astype(np.int32)
    color_index = rng.integers(0, P, n).astype(np.int32)
    px = list(rng.permutation(n))
    pixels = lambda k: np.array([px.pop() for _ in range(k)])
    for rows_of in (lambda: 0, lambda: int(live_rows[-1]) if live_rows.size else 0, lambda: -1, lambda: P - 1, lambda: P + 7, lambda: 10 ** 6, lambda: -3,
                    lambda: int(spare_rows[0]) if spare_rows.size else 0):
        p = pixels(12)
        depth_index[p] = color_index[p] = rows_of()
        dclass[p[:6]], cclass[p[:6]] = 1, 1
    gt_depth[pixels(60)] = 0.0
    if named:
        p = pixels(40)
        depth_index[p] = color_index[p] = named["many_pixels"][0]
        dclass[p], cclass[p] = 0, rng.choice(2, 40)
        for k, d, c in (("depth_strike", 1, 0), ("color_strike", 0, 1), ("both_strikes", 1, 1), ("unstable_struck", 1, 1),
                        ("promoted_and_released", 0, 1)):
            p = pixels(2)
            depth_index[p] = color_index[p] = named[k][0]
            dclass[p], cclass[p] = d, c
    u = rng.random(n).astype(np.float32)
    render_depth = np.where(dclass == 0, gt_depth - 0.05 * u, np.where(dclass == 1, gt_depth - (0.4 + 0.2 * u), gt_depth + 0.5)).astype(np.float32)
    gt_color = rng.uniform(0.3, 0.7, (3, n)).astype(np.float32)
    sign = rng.choice([-1.0, 1.0], (3, n)).astype(np.float32)
    mag = np.where(cclass[None, :] == 0, 0.01 * rng.random((3, n)), rng.uniform(0.15, 0.25, (3, n))).astype(np.float32)
    render_color = (gt_color + sign * mag).astype(np.float32)
    t = torch.from_numpy
    return dict(state={k: t(v) for k, v in state.items()}, gt_color=t(gt_color).reshape(3, H, W), gt_depth=t(gt_depth).reshape(1, H, W),
                render_color=t(render_color).reshape(3, H, W), render_depth=t(render_depth).reshape(1, H, W),
                depth_index=t(depth_index).reshape(1, H, W), color_index=t(color_index).reshape(1, H, W), tick=tick, named=named,
                kw=dict(THRESHOLDS, unstable_time_window=window, delete_thresh=delete_thresh, park=torch.from_numpy(PARK)))


FRAME = ("gt_color", "gt_depth", "render_color", "render_depth", "depth_index", "color_index")

SEQUENCE_STEPS = 12


def sequence_case():
    """The twelve-step sequence: delete_thresh = 3, a window of 8 ticks, the same frame every step.  Scripted on top of the random map:
    `color_row` (stable, struck on colour every step: released at step 2; its confidence is bumped after step 3, so step 4 promotes and
    releases it again), `depth_row` (stable, struck on depth every step: deleted at step 2), `late_row` (unstable; bumped after step 1:
    promoted at step 2)."""
    case = make_case(4242, delete_thresh=3, window=8)
    s, nm = case["state"], case["named"]
    color_row, depth_row, late_row = int(nm["color_strike"][0]), int(nm["depth_strike"][0]), int(nm["at_thres"][0])
    s["color_error_counter"][color_row] = s["depth_error_counter"][color_row] = 0
    s["depth_error_counter"][depth_row] = s["color_error_counter"][depth_row] = 0
    s["confidence"][late_row], s["add_tick"][late_row] = 1.0, case["tick"]
    for r in (color_row, depth_row):  # nothing but the scripted strike reaches them
        for m in ("depth_index", "color_index"):
            flat = case[m].reshape(-1)
            flat[flat == r] = -1
    case["depth_index"].reshape(-1)[0] = depth_row
    case["color_index"].reshape(-1)[1] = color_row
    case["gt_depth"].reshape(-1)[0:2] = 2.0
    case["render_depth"].reshape(-1)[0:2] = torch.tensor([1.5, 2.0])
    case["render_color"].reshape(3, -1)[:, 0] = case["gt_color"].reshape(3, -1)[:, 0]
    case["render_color"].reshape(3, -1)[:, 1] = case["gt_color"].reshape(3, -1)[:, 1] + 0.2
    case["scripted"] = dict(color_row=color_row, depth_row=depth_row, late_row=late_row)
    return case


def sequence_bump(step, scripted):
    """(rows, confidence) the test writes into the state AFTER step `step` (on the GPU state and on the oracle's alike), or None."""
    thres = THRESHOLDS["stable_confidence_thres"]
    if step == 1:
        return [scripted["late_row"]], thres + 2
    if step == 3:
        return [scripted["color_row"]], thres + 5
    return None
