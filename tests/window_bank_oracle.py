"""dqo_window_bank_arm / dqo_window_bank_select (include/dqo_raster.h, csrc/map_window_bank.hip) restated in numpy, statement by
statement: the state words, the copy-or-skip rule per group, the lost-frame log and the overrun.  No GPU, no library.

A bank is a dict of arrays with K_cap leading rows: camera float32 [K,40], gt_color float32 [K,3,H,W], gt_depth float32 [K,1,H,W],
render_mask uint8 [K,H,W], tile_mask int32 [K,gy,gx] and, with a gate, pixel_object int32 [K,H,W] and tile_objects int64 [K,gy*gx].
A destination is a dict of one slot's worth each: bg [3], viewmatrix [16], projmatrix [16], campos [3] and the other parts by the bank's
names.  select() writes the destination in place and returns the names it wrote."""
import numpy as np

WORDS = ("cursor", "n", "prev_k", "prev_m", "force", "overrun", "lost_count")  # behind the ticket, in this order
CAMERA = (("bg", 0, 3), ("viewmatrix", 3, 19), ("projmatrix", 19, 35), ("campos", 35, 38))  # floats of a camera row; 38, 39: pad
CAMERA_GROUP = ("gt_color", "gt_depth", "pixel_object", "tile_objects")  # with the camera row: slot k
MASK_GROUP = ("render_mask", "tile_mask")  # slot m


def arm(n):
    """The state after dqo_window_bank_arm(state, n)."""
    assert n >= 0
    return dict(cursor=0, n=int(n), prev_k=-1, prev_m=-1, force=1, overrun=0, lost_count=0)


def state_words(state):
    return np.array([state[w] for w in WORDS], np.int32)


def select(state, bank, dst, schedule, lost, overflow=False, list_entries=None):
    """One dqo_window_bank_select launch.  schedule: int [n_list, 2]; lost: int32 [n_list], written in place; overflow: whether the
    render header's overflow word is set when the launch runs; list_entries: DqoWindowBank.n (default: the schedule's rows)."""
    schedule = np.asarray(schedule, np.int64).reshape(-1, 2)
    entries = schedule.shape[0] if list_entries is None else int(list_entries)
    K_cap = bank["camera"].shape[0]
    c = state["cursor"]
    if c < 0 or c >= state["n"] or c >= entries:
        state["overrun"] = 1
        return []
    k, m = int(schedule[c, 0]), int(schedule[c, 1])
    if not (0 <= k < K_cap and 0 <= m < K_cap):
        state["overrun"] = 2
        return []
    wrote = []
    if state["force"] != 0 or k != state["prev_k"]:
        for name, a, b in CAMERA:
            dst[name][...] = bank["camera"][k, a:b]
            wrote.append(name)
        for name in CAMERA_GROUP:
            if bank.get(name) is not None:
                dst[name][...] = bank[name][k].reshape(dst[name].shape)
                wrote.append(name)
    if state["force"] != 0 or m != state["prev_m"]:
        for name in MASK_GROUP:
            dst[name][...] = bank[name][m].reshape(dst[name].shape)
            wrote.append(name)
    if c > 0 and overflow and state["lost_count"] < entries:
        lost[state["lost_count"]] = c - 1
        state["lost_count"] += 1
    state["prev_k"], state["prev_m"], state["force"], state["cursor"] = k, m, 0, c + 1
    return wrote


def pairs(schedule):
    """A schedule of FusedMapper.window_schedule — ints or (k, m) pairs — as int32 [n, 2]: a plain index k is (k, k)."""
    return np.array([(e if isinstance(e, tuple) else (e, e)) for e in schedule], np.int32).reshape(-1, 2)


def make_bank(rng, K_cap, W, H, gate):
    gy, gx = (H + 15) // 16, (W + 15) // 16
    bank = dict(camera=rng.normal(size=(K_cap, 40)).astype(np.float32), gt_color=rng.uniform(size=(K_cap, 3, H, W)).astype(np.float32),
                gt_depth=rng.uniform(0.5, 4.0, size=(K_cap, 1, H, W)).astype(np.float32),
                render_mask=(rng.uniform(size=(K_cap, H, W)) < 0.7).astype(np.uint8),
                tile_mask=rng.integers(0, 2, size=(K_cap, gy, gx)).astype(np.int32), pixel_object=None, tile_objects=None)
    if gate:
        bank["pixel_object"] = rng.integers(-1, 64, size=(K_cap, H, W)).astype(np.int32)
        bank["tile_objects"] = rng.integers(-(1 << 62), 1 << 62, size=(K_cap, gy * gx)).astype(np.int64)
    return bank


def make_destination(bank, fill=0):
    dst = {name: np.full((b - a,), fill, np.float32) for name, a, b in CAMERA}
    for name in CAMERA_GROUP + MASK_GROUP:
        if bank.get(name) is not None:
            dst[name] = np.full(bank[name].shape[1:], fill, bank[name].dtype)
    return dst
