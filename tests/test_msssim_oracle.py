"""CPU: the MS-SSIM restatement (tests/msssim_oracle.py) against what can be said about the quantity without the reference's library —
its exact cases, the pooling rule by hand, the size chain — and the argument checks of dqo_eval_ms_ssim, which happen before any launch."""
import numpy as np
import pytest
import torch

from msssim_oracle import level_sizes, ms_ssim_row, pool, uniform_pair

USED = list(range(19))


def test_identical_images_give_exactly_one():
    a, _ = uniform_pair(203, 177, 3)
    for dtype in (torch.float64, torch.float32):
        row = ms_ssim_row(a, a, dtype)
        assert (row[USED] == 1.0).all(), row
        assert np.isnan(row[19])


def test_a_negated_image_gives_exactly_zero():
    a, _ = uniform_pair(203, 177, 3)
    row = ms_ssim_row(a, 1.0 - a)
    assert row[0] == 0.0 and (row[1:4] == 0.0).all()
    assert (row[4:16] == 0.0).all(), row  # levels 0..3: cs < 0 everywhere, clamped


def test_pooling_rule_by_hand():
    """161 x 177, odd in both directions: output j averages inputs 2 j - 1 and 2 j, index -1 is a zero, the divisor is 4."""
    rng = np.random.default_rng(5)
    W, H = 161, 177
    x = rng.uniform(0, 1, (H, W))
    oh, ow = H // 2 + H % 2, W // 2 + W % 2
    want = np.zeros((oh, ow))
    for j in range(oh):
        for i in range(ow):
            s = 0.0
            for dy in (0, 1):
                for dx in (0, 1):
                    yy, xx = 2 * j - H % 2 + dy, 2 * i - W % 2 + dx
                    if yy >= 0 and xx >= 0:
                        s += x[yy, xx]
            want[j, i] = s / 4
    got = pool(torch.tensor(x)[None, None])[0, 0].numpy()
    assert got.shape == (89, 81)
    assert np.abs(got - want).max() < 1e-15
    # ... and an even side starts at input 0
    e = rng.uniform(0, 1, (164, 176))
    ge = pool(torch.tensor(e)[None, None])[0, 0].numpy()
    assert ge.shape == (82, 88)
    assert np.abs(ge - (e[0::2, 0::2] + e[0::2, 1::2] + e[1::2, 0::2] + e[1::2, 1::2]) / 4).max() < 1e-15


def test_size_chain():
    assert [s[0] for s in level_sizes(161, 161)] == [161, 81, 41, 21, 11]
    assert level_sizes(1200, 680) == [(1200, 680), (600, 340), (300, 170), (150, 85), (75, 43)]
    assert level_sizes(203, 177) == [(203, 177), (102, 89), (51, 45), (26, 23), (13, 12)]


@pytest.fixture(scope="module")
def native():
    import __graft_entry__ as g
    g.build_hip()
    import _dqo_native
    return _dqo_native


def test_size_query_follows_the_references_assertion(native):
    lib = native.lib()
    assert lib.dqo_eval_ms_ssim_workspace_bytes(160, 300) == 0
    assert lib.dqo_eval_ms_ssim_workspace_bytes(300, 160) == 0
    assert lib.dqo_eval_ms_ssim_workspace_bytes(161, 161) > 0
    assert lib.dqo_eval_ms_ssim_workspace_bytes(-5, 300) == 0
    assert lib.dqo_eval_ms_ssim_workspace_bytes(65536, 65536) == 0
    n = lib.dqo_eval_ms_ssim_workspace_bytes(1200, 680)
    # the pooled levels 1..4 of both images: about 2 * 3 * H W / 3 floats
    assert 4 * 2 * 1200 * 680 < n < 4 * 2 * 1200 * 680 * 1.2 and n % 256 == 0


def test_argument_errors_come_before_any_launch(native):
    """No GPU here: every one of these returns before anything is launched (the pointers are never followed)."""
    lib = native.lib()
    n = lib.dqo_eval_ms_ssim_workspace_bytes(300, 200)
    assert lib.dqo_eval_ms_ssim(300, 200, 1, 1, None, None, 0, 1, n, None) == -1 and b"null" in lib.dqo_last_error()
    assert lib.dqo_eval_ms_ssim(300, 200, None, 1, None, 1, 0, 1, n, None) == -1 and b"null" in lib.dqo_last_error()
    assert lib.dqo_eval_ms_ssim(300, 160, 1, 1, None, 1, 0, 1, n, None) == -1 and b"160" in lib.dqo_last_error()
    assert lib.dqo_eval_ms_ssim(300, 200, 1, 1, None, 1, -1, 1, n, None) == -1 and b"row" in lib.dqo_last_error()
    assert lib.dqo_eval_ms_ssim(300, 200, 1, 1, None, 1, 0, 1, n - 1, None) == -2 and b"workspace" in lib.dqo_last_error()
    assert lib.dqo_eval_ms_ssim(300, 200, 1, 1, None, 1, 0, None, n, None) == -2 and b"workspace" in lib.dqo_last_error()


def test_python_surface(native):
    import dqo_eval
    assert len(dqo_eval.MS_ROW) == 20 and dqo_eval.MS_ROW[:4] == ("ms_ssim", "ms_r", "ms_g", "ms_b")
    assert dqo_eval.MS_ROW.index("F2_g") == 4 + 3 * 2 + 1
    with pytest.raises(RuntimeError, match="no CPU path"):
        dqo_eval.ms_ssim(torch.zeros(3, 200, 300), torch.zeros(3, 200, 300))
    with pytest.raises(RuntimeError, match="161"):
        dqo_eval.ms_ssim_workspace(300, 160, "cpu")
    # ms_row=None: exactly the dict of before
    row = torch.arange(8, dtype=torch.float32)
    assert dqo_eval.eval_picture_dict(row) == {"valid_pixel_ratio": 3.0, "depth_loss": 2.0, "normal_loss": 0, "psnr": 0.0, "ssim": 4.0,
                                               "color_loss": 1.0}
    both = torch.arange(28, dtype=torch.float32) + 100
    for r, m in ((both[:8], both[8:]), (row, both[8:])):  # views of one tensor: one read; two tensors: two
        d = dqo_eval.eval_picture_dict(r, ms_row=m)
        assert d["ssim"] == 108.0 and d["ssim_single_scale"] == float(r[4]) and d["psnr"] == float(r[0]) and "lpips" not in d
