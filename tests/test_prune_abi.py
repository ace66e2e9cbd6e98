"""CPU-side checks of the floater-pruning entry points (dqo_prune_workspace_bytes, dqo_prune_cameras, dqo_prune_touch, dqo_prune_rows;
csrc/map_prune.hip): the symbols are declared, exported and bound, the size query behaves, every argument error is reported before
anything is launched (-1 for bad arguments, -2 for a short workspace; no GPU here), and the Python surface is the documented one."""
import ctypes
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dqo_prune_workspace_bytes", "dqo_prune_cameras", "dqo_prune_touch", "dqo_prune_rows")
FAKE = 0x10000  # a non-NULL address that is never dereferenced: every call below fails its checks before any launch
BIG = 1 << 40


@pytest.fixture(scope="module")
def native():
    import __graft_entry__ as g
    g.build_hip()
    import _dqo_native
    return _dqo_native


def test_symbols_are_declared_exported_and_bound(native):
    hdr = open(os.path.join(ROOT, "include", "dqo_raster.h")).read()
    lib = ctypes.CDLL(native.LIB_PATH)
    for s in NEW:
        assert s + "(" in hdr and hasattr(lib, s) and s in native.EXPORTS
        assert getattr(native.lib(), s).argtypes
    assert native.lib().dqo_prune_workspace_bytes.restype is ctypes.c_size_t
    for cite in ("mapper.py:424-529", "gaussian_pointcloud.py:52, 230-231, 277-279, 435", ":471-481", ":424-466", "cameras.py:169-183", ":431-443",
                 ":506-508", ":509-527", ":510-515", ":529"):
        assert cite in hdr, cite  # the reference lines the entries replace
    mk = open(os.path.join(ROOT, "dqo-map_amd", "csrc", "Makefile")).read()
    assert " map_prune.hip" in mk and "../build/map_prune.o: HIPFLAGS += -ffp-contract=off" in mk
    src = open(os.path.join(ROOT, "dqo-map_amd", "csrc", "map_prune.hip")).read()
    assert src.index("__global__") < src.index('extern "C"')  # the entry points sit beside their launches, behind them


def test_the_abi_did_not_move(native):
    hdr = open(os.path.join(ROOT, "include", "dqo_raster.h")).read()
    L = native.lib()
    assert L.dqo_abi_version() == 5 and "#define DQO_ABI_VERSION 5" in hdr
    assert L.dqo_abi_sizeof(13) == 0 and L.dqo_abi_sizeof(16) == 0  # (no new struct: the entries take plain arguments)
    assert L.dqo_abi_sizeof(14) == ctypes.sizeof(native.DqoLifecycle) and L.dqo_abi_sizeof(15) == ctypes.sizeof(native.DqoGrowthSample)


def test_workspace_bytes(native):
    f = native.lib().dqo_prune_workspace_bytes
    assert f(0) > 0 and f(0) % 256 == 0 and f(-5) == f(0)
    assert f(1) == f(0) + 256 and f(64) == f(0) + 256 and f(65) == f(0) + 512  # one uint32 word per row behind the head
    assert f(70100) >= f(0) + 4 * 70100 and f(70100) % 256 == 0


def _cameras(native, **kw):
    a = dict(H=36, W=50, viewmatrix=FAKE, projection=FAKE, depth=FAKE, pixel=7, cos=1.0, sin=0.0, view=FAKE, proj=FAKE, focal=FAKE)
    a.update(kw)
    L = native.lib()
    rc = L.dqo_prune_cameras(a["H"], a["W"], a["viewmatrix"], a["projection"], a["depth"], a["pixel"], a["cos"], a["sin"], a["view"], a["proj"],
                             a["focal"], None)
    return rc, L.dqo_last_error().decode()


@pytest.mark.parametrize("case, kw, msg", [
    ("H 0", dict(H=0), "bad image size"),
    ("W negative", dict(W=-3), "bad image size"),
    ("image too large", dict(H=1 << 16, W=1 << 15), "bad image size"),
    ("null viewmatrix", dict(viewmatrix=None), "null viewmatrix"),
    ("null projection", dict(projection=None), "null viewmatrix / projection"),
    ("null depth", dict(depth=None), "null viewmatrix / projection / depth"),
    ("null out view", dict(view=None), "null output"),
    ("null out proj", dict(proj=None), "null output"),
    ("null out focal", dict(focal=None), "null output"),
    ("pixel negative", dict(pixel=-1), "pixel -1 outside the 36 x 50 image"),
    ("pixel one past the image", dict(pixel=36 * 50), "pixel 1800 outside"),
    ("pixel far past int32", dict(pixel=1 << 33), "outside"),
])
def test_cameras_validation_before_launch(native, case, kw, msg):
    rc, err = _cameras(native, **kw)
    assert rc == -1 and re.search(msg, err), (rc, err)


def test_touch_validation_before_launch(native):
    L = native.lib()
    need = L.dqo_prune_workspace_bytes(600)
    assert L.dqo_prune_touch(-1, FAKE, None, FAKE, BIG, None) == -1 and b"bad P" in L.dqo_last_error()
    assert L.dqo_prune_touch(600, None, None, FAKE, BIG, None) == -1 and b"null n_touched" in L.dqo_last_error()
    assert L.dqo_prune_touch(600, FAKE, FAKE, FAKE, need - 1, None) == -2
    assert L.dqo_last_error().decode() == f"prune workspace too small ({need - 1} < {need})"
    assert L.dqo_prune_touch(600, FAKE, FAKE, None, BIG, None) == -2 and b"workspace too small" in L.dqo_last_error()
    assert L.dqo_prune_touch(0, None, None, None, 0, None) == 0  # an empty map: nothing to launch


def _rows(native, P=600, lo=3, hi=4, ws=FAKE, ws_bytes=BIG, stats=FAKE, **null):
    names = ("xyz", "opacity_raw", "scaling_raw", "confidence", "alive", "row_flags", "stable", "add_tick", "depth_error_counter",
             "color_error_counter", "frame_id", "park")
    assert set(null) <= set(names)
    L = native.lib()
    rc = L.dqo_prune_rows(P, *[None if n in null else FAKE for n in names], lo, hi, ws, ws_bytes, stats, None)
    return rc, L.dqo_last_error().decode()


def test_rows_validation_before_launch(native):
    need = native.lib().dqo_prune_workspace_bytes(600)
    rc, err = _rows(native, P=-1)
    assert rc == -1 and "bad P" in err
    rc, err = _rows(native, lo=5, hi=4)
    assert rc == -1 and err == "bad window (5, 4]"
    rc, err = _rows(native, stats=None)
    assert rc == -1 and "null stats" in err
    for name in ("xyz", "opacity_raw", "scaling_raw", "confidence", "alive", "row_flags", "stable", "add_tick", "depth_error_counter",
                 "color_error_counter", "frame_id", "park"):
        rc, err = _rows(native, **{name: True})
        assert rc == -1 and "null per-Gaussian buffer / park" in err, name
    rc, err = _rows(native, ws_bytes=need - 1)
    assert rc == -2 and err == f"prune workspace too small ({need - 1} < {need})"
    rc, err = _rows(native, ws=None)
    assert rc == -2 and "workspace too small" in err


def test_python_surface(native):
    import torch
    import dqo_mapgrowth as mg
    from dqo_harness import fused_mapping as F
    assert list(inspect.signature(mg.prune_cameras).parameters) == ["viewmatrix", "projection", "depth_map", "pixel", "theta_deg", "out"]
    assert inspect.signature(mg.prune_cameras).parameters["theta_deg"].default == 3.0
    assert list(inspect.signature(mg.prune_step).parameters) == ["state", "touched_ws", "window", "park", "stats"]
    assert mg.PRUNE_STATE[:-1] == mg.LIFECYCLE_STATE and mg.PRUNE_STATE[-1] == ("frame_id", torch.int32, 1)
    assert mg.PRUNE_STATS[:6] == ("window_rows", "deleted_unstable", "deleted_stable", "valid_renders", "skipped", "alive_left") and len(mg.PRUNE_STATS) == 8
    sig = inspect.signature(F.FusedMapper.prune_floaters)
    assert list(sig.parameters) == ["self", "depth_map", "window", "projection", "settings", "tile_mask", "theta_deg", "centre"]
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("projection", "settings", "tile_mask", "theta_deg", "centre"))
    assert (sig.parameters["theta_deg"].default, sig.parameters["centre"].default) == (3.0, "reference")
    assert inspect.signature(F.FusedMapper.track_lifecycle).parameters["frame_id"].default is None
    assert inspect.signature(F.FusedMapper.grow).parameters["frame_id"].default is None
    assert inspect.signature(F.FusedMapper._maintain_render).parameters["tile_mask"].default is None
    col = [b for b in F._ROW_BUFFERS if b.name == "frame_id"]
    assert len(col) == 1 and (col[0].group, col[0].spare, col[0].freed, col[0].live) == ("meta", 0, True, 0)
    with pytest.raises(RuntimeError, match="GPU"):
        mg.prune_cameras(torch.eye(4), torch.eye(4), torch.ones(4, 4), 0)
