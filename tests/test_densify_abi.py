"""CPU-side checks of dqo_surfel_densify (include/dqo_raster.h; dqo_eval.densify): both symbols are declared and exported, and every
argument error is reported before anything is launched (no GPU here)."""
import ctypes
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dqo_surfel_densify_workspace_bytes", "dqo_surfel_densify")
FAKE = 0x10000  # a non-NULL address that is never dereferenced: every call below fails its checks before any launch


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


def _call(native, **kw):
    a = dict(P=100, xyz=FAKE, scaling_raw=FAKE, rotation_raw=FAKE, row_keep=None, circle_num=30, levels=5, sigma=1, circle_cs=FAKE, frame=0,
             seed=0, cap=1000, points=FAKE, normals=None, index=None, keep=FAKE, header=FAKE, ws=FAKE, ws_bytes=1 << 40)
    a.update(kw)
    L = native.lib()
    rc = L.dqo_surfel_densify(a["P"], a["xyz"], a["scaling_raw"], a["rotation_raw"], a["row_keep"], a["circle_num"], a["levels"], a["sigma"],
                              a["circle_cs"], a["frame"], a["seed"], a["cap"], a["points"], a["normals"], a["index"], a["keep"], a["header"],
                              a["ws"], a["ws_bytes"], None)
    return rc, L.dqo_last_error().decode()


@pytest.mark.parametrize("case, kw, msg", [
    ("null xyz", dict(xyz=None), "null pointer"),
    ("null scaling", dict(scaling_raw=None), "null pointer"),
    ("null rotation", dict(rotation_raw=None), "null pointer"),
    ("null table", dict(circle_cs=None), "null pointer"),
    ("null points", dict(points=None), "null pointer"),
    ("null keep", dict(keep=None), "null pointer"),
    ("null header", dict(header=None), "null pointer"),
    ("circle_num 0", dict(circle_num=0), "at least 1"),
    ("levels 0", dict(levels=0), "at least 1"),
    ("sigma 0", dict(sigma=0), "at least 1"),
    ("sigma negative", dict(sigma=-2), "at least 1"),
    ("circle_num 1025", dict(circle_num=1025, levels=1), "at most 1024"),
    ("M 65536", dict(circle_num=1024, levels=64, sigma=1), "at most 65535"),
    ("M overflows int32", dict(circle_num=1024, levels=1 << 20, sigma=1 << 20), "at most 65535"),
    ("P * M = 2^32", dict(P=1 << 20, circle_num=1024, levels=4, sigma=1), "below 2\\^32"),
    ("cap 0", dict(cap=0), "bad capacity"),
    ("cap negative", dict(cap=-5), "bad capacity"),
    ("P 0", dict(P=0), "bad row count"),
    ("frame 2", dict(frame=2), "bad frame"),
])
def test_validation_errors_without_a_gpu(native, case, kw, msg):
    rc, err = _call(native, **kw)
    assert rc == -1 and re.search(msg, err), (rc, err)  # DQO_ERR_INVALID_ARG


def test_short_or_missing_workspace(native):
    L = native.lib()
    need = L.dqo_surfel_densify_workspace_bytes(100, 30, 5, 1)
    assert need > 0
    for kw in (dict(ws_bytes=need - 1), dict(ws=None)):
        rc, err = _call(native, **kw)
        assert rc == -2 and "workspace too small" in err, (rc, err)  # DQO_ERR_WORKSPACE


def test_workspace_bytes(native):
    L = native.lib()
    f = L.dqo_surfel_densify_workspace_bytes
    assert f(1, 1, 1, 1) > 0 and f(500000, 30, 5, 1) > f(100, 30, 5, 1)
    assert f((1 << 20) - 1, 1024, 4, 1) > 0  # the largest P * M: 2^32 - 4096
    for bad in ((0, 30, 5, 1), (-1, 30, 5, 1), (100, 0, 5, 1), (100, 30, 0, 1), (100, 30, 5, 0), (100, 1025, 1, 1), (100, 1024, 64, 1),
                (1 << 20, 1024, 4, 1), (100, 1024, 1 << 20, 1 << 20)):
        assert f(*bad) == 0, bad


def test_python_entry(native):
    import dqo_eval
    from dqo_harness.fused_mapping import FusedMapper
    sig = inspect.signature(dqo_eval.densify)
    assert list(sig.parameters) == ["xyz", "scaling_raw", "rotation_raw", "sigma", "circle_num", "levels", "theta", "keep", "sample_nums",
                                    "seed", "frame", "want_normals", "want_index", "workspace_buffer"]
    d = {k: p.default for k, p in sig.parameters.items()}
    assert (d["sigma"], d["circle_num"], d["levels"], d["frame"], d["seed"], d["sample_nums"]) == (1, 30, 5, "reference", 0, None)
    assert list(inspect.signature(FusedMapper.evaluate_geometry_densified).parameters) == ["self", "gt_points", "dist_thres", "transform", "out",
                                                                                          "row", "densify"]
    assert inspect.signature(FusedMapper.evaluate_geometry_densified).parameters["densify"].default is None
    assert inspect.signature(FusedMapper.densify).parameters["rows"].default == "stable"
    import torch
    th = dqo_eval.densify_theta(30, seed=4)
    g = torch.Generator(device="cpu")
    g.manual_seed(4)
    assert th.dtype == torch.float32 and torch.equal(th, (torch.rand(1, 30, generator=g) * torch.pi * 2).reshape(-1))
    with pytest.raises(RuntimeError, match="GPU"):
        dqo_eval.densify(torch.zeros(4, 3), torch.zeros(4, 3), torch.zeros(4, 4))
