"""CPU-side checks of the trajectory entry points (dqo_traj_append, dqo_track_world_maps, dqo_eval_ate; csrc/map_traj.hip): the symbols
are declared, exported and bound, the size query behaves, every argument error is reported before anything is launched (-1 for bad
arguments, -2 for a short workspace; no GPU here), and the Python surface is the documented one."""
import ctypes
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dqo_traj_append", "dqo_track_world_maps", "dqo_eval_ate_workspace_bytes", "dqo_eval_ate")
FAKE = 0x10000  # a non-NULL address that is never dereferenced: every call below fails its checks before any launch


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
    assert native.lib().dqo_abi_version() == 5 and "#define DQO_ABI_VERSION 5" in hdr
    assert native.lib().dqo_eval_ate_workspace_bytes.restype is ctypes.c_size_t
    for cite in ("tracker.py:307-339", "cameras.py:165-183", "mapper.py:734-773", "tracker.py:332-337", "utils.py:56-63",
                 "tracker.py:341-346, 426-430", "utils.py:486-532"):
        assert cite in hdr, cite  # the reference lines the entries replace
    mk = open(os.path.join(ROOT, "dqo-map_amd", "csrc", "Makefile")).read()
    assert " map_traj.hip" in mk and "../build/map_traj.o: HIPFLAGS += -ffp-contract=off" in mk


def test_ate_workspace_bytes(native):
    f = native.lib().dqo_eval_ate_workspace_bytes
    assert f(1) > 0 and f(1) % 256 == 0 and f(2000) >= 2000 * 12 * 8 and f(20000) > f(2000)
    assert f(0) == 0 and f(-3) == 0 and f((1 << 24) + 1) == 0 and f(1 << 24) > 0


def _append(native, **kw):
    a = dict(cap=8, pose=FAKE, pose_gt=FAKE, flags=FAKE, kf_metric=FAKE, header=FAKE, rel=FAKE, abs_pose=None, init_pose=None, gt=None,
             projection=FAKE, c2w=FAKE, viewmatrix=FAKE, projmatrix=FAKE, campos=FAKE, guf=5, theta=30.0, trans=0.3)
    a.update(kw)
    L = native.lib()
    rc = L.dqo_traj_append(a["cap"], a["pose"], a["pose_gt"], a["flags"], a["kf_metric"], a["header"], a["rel"], a["abs_pose"], a["init_pose"],
                           a["gt"], a["projection"], a["c2w"], a["viewmatrix"], a["projmatrix"], a["campos"], a["guf"], a["theta"], a["trans"],
                           None)
    return rc, L.dqo_last_error().decode()


@pytest.mark.parametrize("case, kw, msg", [
    ("cap 0", dict(cap=0), "bad capacity"),
    ("cap negative", dict(cap=-1), "bad capacity"),
    ("null pose store", dict(pose=None), "null pointer"),
    ("null flags", dict(flags=None), "null pointer"),
    ("null metric", dict(kf_metric=None), "null pointer"),
    ("null header", dict(header=None), "null pointer"),
    ("no pose at all", dict(rel=None), "one of the relative and the absolute"),
    ("both poses", dict(abs_pose=FAKE), "one of the relative and the absolute"),
    ("gt without store", dict(gt=FAKE, pose_gt=None), "ground-truth"),
    ("projmatrix without projection", dict(projection=None), "projection"),
    ("negative update frame", dict(guf=-1), "gaussian_update_frame"),
])
def test_append_validation_before_launch(native, case, kw, msg):
    rc, err = _append(native, **kw)
    assert rc == -1 and re.search(msg, err), (rc, err)


def test_world_maps_validation_before_launch(native):
    L = native.lib()
    p = FAKE
    for H, W in ((0, 10), (10, 0), (-2, 4), (1 << 15, 1 << 15)):  # H * W < 1, and 3 * H * W past int32
        assert L.dqo_track_world_maps(H, W, p, p, p, p, p, None) == -1 and b"bad image size" in L.dqo_last_error()
    assert L.dqo_track_world_maps(4, 4, None, p, p, p, p, None) == -1
    assert L.dqo_track_world_maps(4, 4, p, p, None, p, p, None) == -1
    assert L.dqo_track_world_maps(4, 4, p, p, p, None, p, None) == -1
    assert L.dqo_track_world_maps(4, 4, p, p, p, p, None, None) == -1 and b"come together" in L.dqo_last_error()
    assert L.dqo_track_world_maps(4, 4, p, None, p, p, p, None) == -1


def test_ate_validation_before_launch(native):
    L = native.lib()
    p, big = FAKE, 1 << 40
    call = lambda N=100, model=p, data=p, ate=p, ws=p, ws_bytes=big, strides=(3, 1, 3, 1): L.dqo_eval_ate(
        N, model, strides[0], strides[1], data, strides[2], strides[3], ate, None, ws, ws_bytes, None)
    for n in (0, -5, (1 << 24) + 1):  # N < 1, N too large
        assert call(N=n) == -1 and b"bad point count" in L.dqo_last_error()
    assert call(model=None) == -1 and b"null pointer" in L.dqo_last_error()  # NULL streams of positions
    assert call(data=None) == -1 and call(ate=None) == -1
    assert call(strides=(3, 1, -16, 4)) == -1 and b"bad stride" in L.dqo_last_error()
    need = L.dqo_eval_ate_workspace_bytes(100)
    assert call(ws_bytes=need - 1) == -2
    assert L.dqo_last_error().decode() == f"ate workspace too small ({need - 1} < {need})"
    assert call(ws=None) == -2 and "workspace too small" in L.dqo_last_error().decode()


def test_python_surface(native):
    import torch
    import dqo_eval
    import dqo_icp
    T = dqo_icp.Trajectory
    sig = inspect.signature(T.__init__)
    assert list(sig.parameters)[:7] == ["self", "capacity", "device", "projection", "gaussian_update_frame", "keyframe_theta_thes",
                                        "keyframe_trans_thes"]
    d = {k: p.default for k, p in sig.parameters.items()}
    assert (d["projection"], d["gaussian_update_frame"], d["keyframe_theta_thes"], d["keyframe_trans_thes"]) == (None, 0, 30.0, 0.3)
    assert list(inspect.signature(T.append).parameters) == ["self", "pose", "relative", "pose_gt"]
    assert inspect.signature(T.append).parameters["relative"].default is True
    assert list(inspect.signature(T.world_maps).parameters) == ["self", "vertex_c", "normal_c", "out"]
    assert list(inspect.signature(T.settings).parameters) == ["self", "template"]
    for name in ("poses", "poses_gt", "keyframe", "is_keyframe", "ate", "overflowed", "save", "__len__"):
        assert callable(getattr(T, name)), name
    assert list(inspect.signature(dqo_eval.eval_ate).parameters)[:3] == ["pose_es", "pose_gt", "out"]
    assert list(inspect.signature(dqo_eval.eval_ate_dict).parameters) == ["curve"]
    with pytest.raises(RuntimeError, match="GPU"):
        dqo_eval.eval_ate(torch.zeros(4, 3, dtype=torch.float64), torch.zeros(4, 3, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="GPU"):
        T(8, "cpu")
    with pytest.raises(RuntimeError, match="GPU"):
        dqo_icp.world_maps(torch.zeros(4, 4, 3), torch.zeros(4, 4, 3), torch.eye(4))
    # the tracker keeps its five methods and signatures (tests/test_track_abi.py pins them): Trajectory is beside it, not in it
    assert not hasattr(dqo_icp.IcpTracker, "append")
