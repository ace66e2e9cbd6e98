"""CPU-side checks of the operator's parameter form (dqo_rast_*_params, include/dqo_raster.h; rasterize_gaussian_params): the symbols are
declared and exported, the struct sizes agree, and every argument error is reported before anything is launched (no GPU here)."""
import ctypes
import inspect
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dqo_rast_forward_prepare_params", "dqo_rast_forward_render_params", "dqo_rast_forward_async_params", "dqo_rast_backward_params")


@pytest.fixture(scope="module")
def native():
    import __graft_entry__ as g
    g.build_hip()
    import _dqo_native
    return _dqo_native


def test_symbols_are_declared_and_exported(native):
    hdr = open(os.path.join(ROOT, "include", "dqo_raster.h")).read()
    lib = ctypes.CDLL(native.LIB_PATH)
    for s in NEW:
        assert s + "(" in hdr and hasattr(lib, s) and s in native.EXPORTS
    assert native.lib().dqo_abi_version() == 5


def test_struct_sizes(native):
    L = native.lib()
    assert L.dqo_abi_sizeof(11) == ctypes.sizeof(native.DqoRastParamInputs)
    assert L.dqo_abi_sizeof(12) == ctypes.sizeof(native.DqoRastParamGrads)
    assert L.dqo_abi_sizeof(13) == 0


FAKE = 0x10000  # a non-NULL address that is never dereferenced: every call below fails its checks before any launch


def _call(native, stage, in_kw=None, pin_kw=None, M=16, D=3, grads_kw=None, pgrads_kw=None):
    N = native
    L = N.lib()
    p = N.DqoRastParams(P=10, D=D, M=M, W=64, H=48, tanfovx=1.0, tanfovy=1.0, scale_modifier=1.0, color_sigma=3.0)
    inp = N.DqoRastInputs(bg=FAKE, means3D=FAKE, viewmatrix=FAKE, projmatrix=FAKE, campos=FAKE, **(in_kw or {}))
    pkw = dict(features_dc=FAKE, features_rest=FAKE, rest=M - 1, opacity_raw=FAKE, scaling_raw=FAKE, rotation_raw=FAKE)
    pkw.update(pin_kw or {})
    pin = N.DqoRastParamInputs(**pkw)
    out = N.DqoRastOutputs(*([FAKE] * 9))
    ctx = N.DqoRastCtx(geom=FAKE, geom_bytes=1 << 30, image=FAKE, image_bytes=1 << 30, binning=FAKE, binning_bytes=1 << 30, inst_capacity=16)
    b = ctypes.byref
    if stage == "prepare":
        rc = L.dqo_rast_forward_prepare_params(b(p), b(inp), b(pin), b(out), b(ctx), None)
    elif stage == "render":
        rc = L.dqo_rast_forward_render_params(b(p), b(inp), b(pin), b(out), b(ctx), None)
    elif stage == "async":
        rc = L.dqo_rast_forward_async_params(b(p), b(inp), b(pin), b(out), b(ctx), None, None, None)
    else:
        g = N.DqoRastGrads(dL_dmeans3D=FAKE, **(grads_kw or {}))
        gkw = dict(dL_dfeatures_dc=FAKE, dL_dfeatures_rest=FAKE, dL_dopacity_raw=FAKE, dL_dscaling_raw=FAKE, dL_drotation_raw=FAKE)
        gkw.update(pgrads_kw or {})
        pg = N.DqoRastParamGrads(**gkw)
        rc = L.dqo_rast_backward_params(b(p), b(inp), b(pin), b(ctx), FAKE, FAKE, FAKE, b(g), b(pg), FAKE, 1 << 40, None)
    return rc, L.dqo_last_error().decode()


STAGES = ["prepare", "render", "async", "backward"]


@pytest.mark.parametrize("stage", STAGES)
@pytest.mark.parametrize("case, kw, msg", [
    ("mixed sh", dict(in_kw=dict(shs=FAKE)), "must be NULL"),
    ("mixed opacities", dict(in_kw=dict(opacities=FAKE)), "must be NULL"),
    ("mixed scales", dict(in_kw=dict(scales=FAKE)), "must be NULL"),
    ("mixed rotations", dict(in_kw=dict(rotations=FAKE)), "must be NULL"),
    ("colors_precomp", dict(in_kw=dict(colors_precomp=FAKE)), "colors_precomp is not supported"),
    ("null dc", dict(pin_kw=dict(features_dc=None)), "null raw parameter"),
    ("null opacity", dict(pin_kw=dict(opacity_raw=None)), "null raw parameter"),
    ("null scaling", dict(pin_kw=dict(scaling_raw=None)), "null raw parameter"),
    ("null rotation", dict(pin_kw=dict(rotation_raw=None)), "null raw parameter"),
    ("null rest", dict(pin_kw=dict(features_rest=None)), "null features_rest"),
    ("too few coefficients", dict(M=9, pin_kw=dict(rest=8)), "degree 3 needs 15"),
    ("M is not 1 + rest", dict(M=16, pin_kw=dict(rest=8)), "must be 1 \\+ rest"),
])
def test_validation_errors_without_a_gpu(native, stage, case, kw, msg):
    import re
    rc, err = _call(native, stage, **kw)
    assert rc == -1 and re.search(msg, err), (rc, err)  # DQO_ERR_INVALID_ARG


@pytest.mark.parametrize("case, kw, msg", [
    ("activated grads given", dict(grads_kw=dict(dL_dsh=FAKE)), "must be NULL"),
    ("colour grads given", dict(grads_kw=dict(dL_dcolors=FAKE)), "must be NULL"),
    ("null raw grad", dict(pgrads_kw=dict(dL_dopacity_raw=None)), "null raw gradient"),
    ("null rest grad", dict(pgrads_kw=dict(dL_dfeatures_rest=None)), "null dL_dfeatures_rest"),
])
def test_backward_gradient_errors(native, case, kw, msg):
    import re
    rc, err = _call(native, "backward", **kw)
    assert rc == -1 and re.search(msg, err), (rc, err)


def test_python_entry(native):
    import diff_gaussian_rasterization_depth as dgr
    sig = inspect.signature(dgr.rasterize_gaussian_params)
    assert list(sig.parameters) == ["means3D", "features_dc", "features_rest", "opacity_raw", "scaling_raw", "rotation_raw", "tile_mask",
                                    "raster_settings"]
    assert list(inspect.signature(dgr.rasterize_gaussians).parameters) == ["means3D", "sh", "colors_precomp", "opacities", "scales",
                                                                           "rotations", "cov3Ds_precomp", "tile_mask", "raster_settings"]
