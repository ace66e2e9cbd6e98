"""CPU: tests/window_bank_oracle.py — the numpy restatement of dqo_window_bank_arm / dqo_window_bank_select the GPU tests are held to —
on hand-written cases: a repeated entry, a (k, m) pair whose halves change separately, force, running past n, a bad index, the log."""
import numpy as np

import window_bank_oracle as O


def _problem(gate=True, K_cap=3, W=33, H=17):
    bank = O.make_bank(np.random.default_rng(1), K_cap, W, H, gate)
    return bank, O.make_destination(bank, fill=9), np.full(8, -7, np.int32)


def _holds(dst, bank, k, m):
    """Whether the destination is exactly slot k's camera group and slot m's mask group."""
    cam = all(np.array_equal(dst[n], bank["camera"][k, a:b]) for n, a, b in O.CAMERA)
    cam = cam and all(np.array_equal(dst[n], bank[n][k].reshape(dst[n].shape)) for n in O.CAMERA_GROUP if bank.get(n) is not None)
    return cam and all(np.array_equal(dst[n], bank[n][m]) for n in O.MASK_GROUP)


def test_arm_and_the_word_order():
    st = O.arm(5)
    assert st == dict(cursor=0, n=5, prev_k=-1, prev_m=-1, force=1, overrun=0, lost_count=0)
    assert O.state_words(st).tolist() == [0, 5, -1, -1, 1, 0, 0] and O.state_words(st).dtype == np.int32
    assert O.pairs([2, (0, 1), 1]).tolist() == [[2, 2], [0, 1], [1, 1]]


def test_a_repeated_entry_copies_nothing():
    bank, dst, lost = _problem()
    st = O.arm(2)
    wrote = O.select(st, bank, dst, [(1, 1), (1, 1)], lost)
    assert set(wrote) == set(dst) and _holds(dst, bank, 1, 1) and st["force"] == 0 and (st["prev_k"], st["prev_m"], st["cursor"]) == (1, 1, 1)
    for a in dst.values():
        a[...] = 0
    assert O.select(st, bank, dst, [(1, 1), (1, 1)], lost) == [] and st["cursor"] == 2
    assert all(not a.any() for a in dst.values())  # untouched


def test_the_halves_of_a_pair_change_separately():
    bank, dst, lost = _problem()
    sched = [(0, 0), (1, 0), (1, 2), (2, 2)]
    st = O.arm(4)
    O.select(st, bank, dst, sched, lost)
    wrote = O.select(st, bank, dst, sched, lost)  # the camera group alone
    assert set(wrote) == {"bg", "viewmatrix", "projmatrix", "campos", "gt_color", "gt_depth", "pixel_object", "tile_objects"}
    assert _holds(dst, bank, 1, 0)
    wrote = O.select(st, bank, dst, sched, lost)  # the mask group alone
    assert set(wrote) == {"render_mask", "tile_mask"} and _holds(dst, bank, 1, 2)
    O.select(st, bank, dst, sched, lost)
    assert _holds(dst, bank, 2, 2) and st["cursor"] == 4 and st["overrun"] == 0 and st["lost_count"] == 0
    # without a gate the gate parts are neither read nor written
    bank, dst, lost = _problem(gate=False)
    assert "pixel_object" not in dst and "tile_objects" not in dst
    assert set(O.select(O.arm(1), bank, dst, [(2, 1)], lost)) == {"bg", "viewmatrix", "projmatrix", "campos", "gt_color", "gt_depth",
                                                                   "render_mask", "tile_mask"}
    assert _holds(dst, bank, 2, 1)


def test_force_copies_an_unchanged_entry_and_is_cleared():
    bank, dst, lost = _problem()
    st = O.arm(3)
    O.select(st, bank, dst, O.pairs([0, 0, 0]), lost)
    bank["gt_color"][0] += 1.0  # the slot is rewritten in place (bank_set, refresh_bank) ...
    bank["render_mask"][0] ^= 1
    assert O.select(st, bank, dst, O.pairs([0, 0, 0]), lost) == [] and not _holds(dst, bank, 0, 0)
    st["force"] = 1  # ... and force makes the next select copy it
    assert set(O.select(st, bank, dst, O.pairs([0, 0, 0]), lost)) == set(dst) and _holds(dst, bank, 0, 0) and st["force"] == 0


def test_running_past_n_and_a_bad_index():
    bank, dst, lost = _problem()
    st = O.arm(1)
    O.select(st, bank, dst, [(2, 2)], lost, overflow=True)
    before = {n: a.copy() for n, a in dst.items()}
    for _ in range(2):
        assert O.select(st, bank, dst, [(2, 2)], lost, overflow=True) == []
        assert st["overrun"] == 1 and st["cursor"] == 1 and st["lost_count"] == 0 and (st["prev_k"], st["prev_m"]) == (2, 2)
    assert all(np.array_equal(before[n], dst[n]) for n in dst) and (lost == -7).all()
    # the lists hold fewer entries than the armed length: the same overrun
    st = O.arm(4)
    assert O.select(st, bank, dst, [(0, 0)] * 4, lost, list_entries=0) == [] and st["overrun"] == 1 and st["cursor"] == 0
    for bad in ((3, 0), (0, 3), (-1, 0), (0, -1)):
        st = O.arm(2)
        assert O.select(st, bank, dst, [bad, (0, 0)], lost) == []
        assert st["overrun"] == 2 and st["cursor"] == 0 and st["force"] == 1 and (st["prev_k"], st["prev_m"]) == (-1, -1)
    assert O.select(O.arm(0), bank, dst, np.zeros((0, 2)), lost) == []


def test_the_lost_frame_log():
    bank, dst, lost = _problem()
    sched = O.pairs([0, 1, 1, 2, 0])
    st = O.arm(5)
    flags = [True, False, True, True, False]  # the header's overflow word when launch c runs: it speaks of position c - 1
    for c in range(5):
        O.select(st, bank, dst, sched, lost, overflow=flags[c])
    assert st["lost_count"] == 2 and lost[:2].tolist() == [1, 2] and (lost[2:] == -7).all()  # (launch 0 has no frame behind it)
