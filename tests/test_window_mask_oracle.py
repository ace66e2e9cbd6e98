"""CPU: the numpy restatement of dqo_window_masks (tests/window_mask_oracle.py) against the reference's recorded results
(tests/golden/tilemask_golden.npz) and against oracle/map_oracle.py where the two must agree."""
import numpy as np

import window_mask_oracle as wo
from oracle import map_oracle as mo
from test_oracle_tilemask import CASES, G, case, topk_mask_agrees


def assert_goldens(masks_of):
    """masks_of(T, render, gt, mode, ratio, k) -> window_mask_oracle.window_masks' dict: the assertions every implementation meets."""
    for c in CASES:
        T, render, gt = case(c)
        h, w = T.shape
        for r in (0.5, 0.25, 0.9):
            got = masks_of(T, render, gt, wo.MODE_LOCAL, r, 0)
            np.testing.assert_array_equal(got["tile_mask"], G[f"{c}_transmission2tilemask_{r}"])
            np.testing.assert_array_equal(got["render_mask"], (T != 1).astype(np.uint8))
            assert np.float32(got["ratio"]) == np.float32((T != 1).sum()) / np.float32(h * w)
        for r in (0.4, 0.1):
            k = wo.top_k(h, w, r)
            got = masks_of(T, render, gt, wo.MODE_ERROR, 0.5, k)
            pooled = got["sums"] / np.float32(256)  # (exact)
            assert topk_mask_agrees(got["tile_mask"], G[f"{c}_colorerror2tilemask_{r}"], pooled, k), (c, r)
            np.testing.assert_array_equal(got["render_mask"], wo.expand_tile_mask(got["tile_mask"], h, w))
            np.testing.assert_allclose(got["sums"], mo.meanpool(G[f"{c}_color_error"], 16).astype(np.float64) * 256, rtol=2e-6, atol=0)
            np.testing.assert_allclose(pooled, G[f"{c}_meanpool"], rtol=2e-6, atol=1e-7)
        got = masks_of(T, render, gt, wo.MODE_FINAL, 0.5, 0)
        assert (got["tile_mask"] == 1).all() and got["tile_mask"].shape == wo.grid(h, w)
        np.testing.assert_array_equal(got["render_mask"], (T != 1).astype(np.uint8))


def test_three_modes_match_reference_goldens():
    assert_goldens(lambda T, render, gt, mode, r, k: wo.window_masks(T, render, gt, mode, r, k))


def test_kernel_order_sums_agree_with_float64_pooling():
    rng = np.random.default_rng(5)
    for h, w in ((1, 1), (17, 5), (131, 203)):
        err = rng.uniform(0, 3, (h, w)).astype(np.float32)
        np.testing.assert_allclose(wo.kernel_tile_sums(err), mo.meanpool(err, 16).astype(np.float64) * 256, rtol=2e-6, atol=0)
    ones = np.ones((16, 32), np.float32)
    assert (wo.kernel_tile_sums(ones) == 256).all()


def test_selection_is_the_stable_descending_order_and_ties_go_to_the_lower_index():
    rng = np.random.default_rng(6)
    err = rng.uniform(0, 1, (131, 203)).astype(np.float32)
    err[:64] = np.float32(0.25)  # four tile rows of equal sums (the last column is ragged: another value)
    sums = wo.kernel_tile_sums(err)
    assert len(np.unique(sums[:4, :-1])) == 1
    for k in (0, 1, 7, 40, 60, sums.size):
        want = np.zeros(sums.size, np.int32)
        want[np.argsort(-sums.reshape(-1), kind="stable")[:k]] = 1
        got = wo.select_largest(sums, k)
        np.testing.assert_array_equal(got.reshape(-1), want)
        assert got.sum() == k
        ref, pooled, kk = mo.colorerror2tilemask(err, 16, k / sums.size + 1e-9)
        if kk == k:
            assert topk_mask_agrees(got, ref, pooled, k)
    zero = np.zeros((3, 5), np.float32)
    np.testing.assert_array_equal(wo.select_largest(zero, 4).reshape(-1), [1, 1, 1, 1] + [0] * 11)


def test_a_nan_sum_lies_above_every_number():
    sums = np.array([[1.0, np.inf, 3.0], [np.nan, 0.0, 2.0]], np.float32)
    np.testing.assert_array_equal(wo.select_largest(sums, 1), [[0, 0, 0], [1, 0, 0]])
    np.testing.assert_array_equal(wo.select_largest(sums, 3), [[0, 1, 1], [1, 0, 0]])
    render = np.full((3, 16, 32), 0.5, np.float32)
    gt = render.copy()
    gt[1, 3, 20] = np.nan
    got = wo.window_masks(None, render, gt, wo.MODE_ERROR, k=1)
    np.testing.assert_array_equal(got["tile_mask"], [[0, 1]])
    assert got["render_mask"][:, 16:].all() and not got["render_mask"][:, :16].any() and got["ratio"] == np.float32(0.5)


def test_expansion_ratio_and_zeroed_pixels():
    rng = np.random.default_rng(7)
    h, w = 37, 50
    render, gt = rng.uniform(0, 1, (3, h, w)).astype(np.float32), rng.uniform(0, 1, (3, h, w)).astype(np.float32)
    render[:, :16, :16] = 0  # a tile whose rendered colour sums to 0 everywhere: no error, whatever the target
    got = wo.window_masks(None, render, gt, wo.MODE_ERROR, k=11)
    assert got["sums"][0, 0] == 0 and got["tile_mask"][0, 0] == 0 and got["tile_mask"].sum() == 11
    up = np.zeros((h, w), np.uint8)
    for ty, tx in zip(*np.nonzero(got["tile_mask"])):
        up[16 * ty:16 * ty + 16, 16 * tx:16 * tx + 16] = 1
    np.testing.assert_array_equal(got["render_mask"], up)
    assert got["ratio"] == np.float32(up.sum()) / np.float32(h * w)
    T = np.where(rng.uniform(size=(h, w)) < 0.5, np.float32(1), rng.uniform(0, 1, (h, w)).astype(np.float32))
    loc = wo.window_masks(T, mode=wo.MODE_LOCAL, tile_mask_ratio=0.5)
    cnt = np.zeros(wo.grid(h, w))
    for ty in range(cnt.shape[0]):
        for tx in range(cnt.shape[1]):
            cnt[ty, tx] = (T[16 * ty:16 * ty + 16, 16 * tx:16 * tx + 16] != 1).sum()
    np.testing.assert_array_equal(loc["tile_mask"], (cnt / 256 > 0.5).astype(np.int32))  # always divided by 256: ragged tiles rarely pass
