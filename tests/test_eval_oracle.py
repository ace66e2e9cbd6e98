"""CPU: the keyframe-evaluation oracle (tests/eval_oracle.py, float64) against what the reference's own functions returned for the five
cases of tests/golden/eval_golden.npz (tests/golden/make_eval_golden.py: psnr / l1_loss / ssim / mse of utils/loss_utils.py and the depth
statements of SLAM/eval.py:115-126, torch float32 on the CPU) — and the two new C-ABI symbols.

Bars: psnr (dB), color_loss, depth_loss and ssim within 1e-4 absolute.  The recorded side is torch float32 means over 3 072 - 9 216
elements, whose summation error is about log2(n) 2^-24 ~ 1e-6 relative: 1e-4 leaves two orders of margin — an oracle that misses it
restates the reference wrongly.  The mean squared errors (not a key of the reference's dict; recorded with its `mse`) within 1e-5
relative: the same float32 mean plus one float32 rounding per square, ten times over.  valid_pixel_ratio is the float32 quotient of
two integers on both sides: exact.  inf and NaN sit in the same places."""
import ctypes
import os
import re

import numpy as np
import pytest

from eval_oracle import INPUTS, ROW, eval_oracle, fixture_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ABS_BAR = 1e-4  # psnr, color_loss, depth_loss, ssim
MSE_REL_BAR = 1e-5


def load_fixture():
    g = np.load(os.path.join(ROOT, "tests", "golden", "eval_golden.npz"))
    return fixture_cases(g), np.asarray(g["want"], np.float32)


def assert_row(got, want, what, abs_bar=ABS_BAR, mse_rel_bar=MSE_REL_BAR, slots=range(8)):
    """got / want: [8] in ROW order.  Prints each figure before it asserts."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    for k in slots:
        g, w = got[k], want[k]
        print(f"{what} {ROW[k]:18s} got {g!r} want {w!r}")
        if not np.isfinite(w):
            assert (np.isnan(g) and np.isnan(w)) or g == w, (what, ROW[k], g, w)
        elif k == 3:
            assert np.float32(g) == np.float32(w), (what, ROW[k], g, w)
        elif k >= 5:
            assert abs(g - w) <= mse_rel_bar * abs(w), (what, ROW[k], g, w)
        else:
            assert abs(g - w) <= abs_bar, (what, ROW[k], g, w)


def test_the_fixture_shows_what_it_is_meant_to_show():
    cases, want = load_fixture()
    assert [c[0] for c in cases] == ["generic", "identical", "no_valid_pixel", "all_out_of_range", "half_without_hit"] and want.shape == (5, 8)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "eval_golden.npz")) < 120 * 1024
    for _, c, _, _ in cases:
        assert set(c) == set(INPUTS) and c["render"].shape == (3, 48, 64) and c["depth_index"].dtype == np.int32
    w = dict(zip([c[0] for c in cases], want))
    assert np.isfinite(w["generic"]).all() and 0 < w["generic"][3] < 1 and 10 < w["generic"][0] < 60
    assert np.isposinf(w["identical"][0]) and w["identical"][1] == 0 and (w["identical"][5:] == 0).all() and w["identical"][4] == 1
    for name in ("no_valid_pixel", "all_out_of_range"):
        assert np.isnan(w[name][2]) and w[name][3] == 0 and np.isfinite(np.delete(w[name], 2)).all(), name
    assert 0 < w["half_without_hit"][3] < w["generic"][3] and np.isfinite(w["half_without_hit"]).all()
    # a target depth on both sides of the range, holes of the sensor, pixels without a hit
    gd, idx = cases[0][1]["gt_depth"], cases[0][1]["depth_index"]
    assert (gd == 0).any() and ((gd > 0) & (gd < 0.3)).any() and (gd > 5.0).any() and (idx == -1).any() and (idx >= 0).any()


@pytest.mark.parametrize("k", range(5), ids=["generic", "identical", "no_valid_pixel", "all_out_of_range", "half_without_hit"])
def test_oracle_equals_the_reference(k):
    cases, want = load_fixture()
    name, c, lo, hi = cases[k]
    assert_row(eval_oracle(*(c[n] for n in INPUTS), lo, hi), want[k], name)


def test_new_symbols_are_declared_exported_and_bound():
    import __graft_entry__ as g
    g.build_hip()
    import _dqo_native as native
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dqo_raster.h")).read(), flags=re.S)
    lib = ctypes.CDLL(native.LIB_PATH)
    for s in ("dqo_eval_picture_workspace_bytes", "dqo_eval_picture"):
        assert s + "(" in hdr and hasattr(lib, s) and s in native.EXPORTS, s
    L = native.lib()
    assert L.dqo_abi_version() == 5
    small, big = L.dqo_eval_picture_workspace_bytes(64, 48), L.dqo_eval_picture_workspace_bytes(1200, 680)
    assert 0 < small < big and small % 256 == 0 and big % 256 == 0
    assert L.dqo_eval_picture_workspace_bytes(0, 48) == 0 and L.dqo_eval_picture_workspace_bytes(65536, 65536) == 0
    # argument validation happens before any launch: usable without a GPU
    assert L.dqo_eval_picture(0, 48, 1, 1, 1, 1, 1, 0.3, 5.0, None, 1, 0, 1, small, None) == -1 and b"image size" in L.dqo_last_error()
    assert L.dqo_eval_picture(64, 48, 1, 1, 1, 1, 1, 0.3, 5.0, None, None, 0, 1, small, None) == -1 and b"null" in L.dqo_last_error()
    assert L.dqo_eval_picture(64, 48, 1, 1, 1, 1, 1, 0.3, 5.0, None, 1, 0, 1, small - 1, None) == -2 and b"workspace" in L.dqo_last_error()


def test_python_surface():
    import inspect
    import torch
    import dqo_eval
    sig = list(inspect.signature(dqo_eval.eval_picture).parameters)
    assert sig[:8] == ["render_output", "gt_color", "gt_depth", "min_depth", "max_depth", "out", "row", "ssim"]
    assert dqo_eval.ROW == ROW
    for word in ("MS-SSIM", "pytorch_msssim", "LPIPS", "single-scale"):
        assert word in dqo_eval.eval_picture.__doc__, word
    z = lambda *s: torch.zeros(*s)
    with pytest.raises(RuntimeError, match="no CPU path"):
        dqo_eval.eval_picture(dict(render=z(3, 4, 4), depth=z(1, 4, 4), depth_index_map=z(1, 4, 4).int()), z(3, 4, 4), z(1, 4, 4), 0.3, 5.0)
    d = dqo_eval.eval_picture_dict(torch.tensor([30.0, 0.01, 0.02, 0.5, 0.9, 1e-3, 1e-3, 1e-3]))
    assert set(d) == {"valid_pixel_ratio", "depth_loss", "normal_loss", "psnr", "ssim", "color_loss"} and d["normal_loss"] == 0
    assert d["psnr"] == 30.0 and d["valid_pixel_ratio"] == 0.5 and abs(d["ssim"] - 0.9) < 1e-7
    from dqo_harness.fused_mapping import FusedMapper
    assert list(inspect.signature(FusedMapper.evaluate).parameters) == ["self", "frames", "min_depth", "max_depth", "out"]
