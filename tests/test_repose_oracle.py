"""CPU: tests/repose_oracle.py — the numpy restatement of dqo_traj_repose the GPU tests are held to — against values recorded from the
reference's own Camera.updatePose (tests/golden/repose_golden.npz) under test_gpu_traj.py's camera bars: within one float32 ulp of the
float64 truth, and within the reference's own recorded distance from that truth plus that ulp of the reference's tensors.  Then the
entry point's CPU side: declared, exported and bound, the ABI did not move, the structs are the header's, every argument error is
reported before anything is dereferenced or launched (fake pointers; no GPU here), and the Python surface is the documented one."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import repose_oracle as RO
import traj_oracle as TO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "repose_golden.npz"))
FAKE = 0x10000  # a non-NULL address that is never dereferenced: every call below fails its checks before the launch


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


# ---- the oracle against the reference ------------------------------------------------------------------------------------------------

def test_fixture_is_what_the_issue_describes():
    P = G["pose"]
    assert P.shape == (70, 4, 4) and P.dtype == np.float64 and set(G.files) == {"projection", "pose", "view", "full", "view64", "full64",
                                                                                "view_dist", "full_dist"}
    R = P[:, :3, :3]
    assert np.array_equal(R, R.astype(np.float32).astype(np.float64))  # float32-rounded rotations ...
    err = np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max()
    assert 1e-9 < err < 1e-5  # ... orthonormal to float32 only
    assert np.array_equal(P[:, 3], np.tile([0.0, 0.0, 0.0, 1.0], (70, 1)))


def test_oracle_cameras_vs_reference():
    worst_v = worst_f = 0.0
    for i in range(70):
        cam = RO.cameras(G["pose"][i], G["projection"])
        v64, f64 = G["view64"][i], G["full64"][i]
        assert np.all(np.abs(cam["viewmatrix"] - v64) <= ulp32(v64)), i
        assert np.all(np.abs(cam["viewmatrix"] - G["view"][i]) <= G["view_dist"] + ulp32(v64)), i
        assert np.all(np.abs(cam["projmatrix"] - f64) <= ulp32(f64)), i
        assert np.all(np.abs(cam["projmatrix"] - G["full"][i]) <= G["full_dist"] + ulp32(f64)), i
        assert np.array_equal(cam["w2c"], cam["viewmatrix"].T) and np.array_equal(cam["w2c"][3], [0, 0, 0, 1])
        assert np.array_equal(cam["c2w"], G["pose"][i].astype(np.float32)) and np.array_equal(cam["campos"], cam["c2w"][:3, 3])
        worst_v = max(worst_v, np.abs(cam["viewmatrix"] - G["view"][i]).max())
        worst_f = max(worst_f, (np.abs(cam["projmatrix"] - G["full"][i]) / ulp32(f64)).max())
    print("oracle vs Camera.updatePose: viewmatrix", worst_v, "projmatrix", worst_f, "ulp")


def test_oracle_store_and_target_semantics():
    rng = np.random.default_rng(3)
    cap, count = 12, 7
    base = rng.normal(size=(cap, 4, 4))
    base[:, 3] = [0, 0, 0, 1]
    new = G["pose"][:9].copy()
    for n_new, rows in ((0, 0), (1, 1), (6, 6), (7, 7), (9, 7)):
        pose = base.copy()
        targets = [(-1, RO.FIELDS), (count, RO.FIELDS), (cap - 1, RO.FIELDS), (0, ("viewmatrix",)), (0, ("campos", "c2w")), (6, RO.FIELDS)]
        outs, stats = RO.repose(pose, count, new[:n_new], targets, G["projection"])
        assert stats == [rows, 3, 3, 0]
        assert np.array_equal(pose[:rows], new[:rows]) and np.array_equal(pose[rows:], base[rows:])
        assert outs[0] is None and outs[1] is None and outs[2] is None
        src0 = new[0] if n_new > 0 else base[0]
        assert set(outs[3]) == {"viewmatrix"} and np.array_equal(outs[3]["viewmatrix"], TO.camera(src0)["viewmatrix"])
        assert set(outs[4]) == {"campos", "c2w"} and np.array_equal(outs[4]["c2w"], src0.astype(np.float32))
        src6 = new[6] if n_new > 6 else base[6]  # a row at or beyond n_new keeps its pose, and its camera comes from the store
        assert np.array_equal(outs[5]["projmatrix"], TO.camera(src6, G["projection"])["projmatrix"])
    pose = base.copy()
    outs, stats = RO.repose(pose, 99, None, [(cap - 1, ("w2c",))])  # the count is clipped to the capacity; no new poses
    assert stats == [0, 1, 0, 0] and np.array_equal(pose, base) and set(outs[0]) == {"w2c"}


# ---- the entry point's CPU side ------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def native():
    import __graft_entry__ as g
    g.build_hip()
    import _dqo_native
    return _dqo_native


def _header():
    return open(os.path.join(ROOT, "include", "dqo_raster.h")).read()


def test_symbol_is_declared_exported_and_bound(native):
    hdr = _header()
    lib = ctypes.CDLL(native.LIB_PATH)
    L = native.lib()
    assert "dqo_traj_repose(" in hdr and hasattr(lib, "dqo_traj_repose") and "dqo_traj_repose" in native.EXPORTS
    assert L.dqo_traj_repose.argtypes[1] is ctypes.c_void_p
    mk = open(os.path.join(ROOT, "dqo-map_amd", "csrc", "Makefile")).read()
    assert " map_repose.hip" in mk and "../build/map_repose.o: HIPFLAGS += -ffp-contract=off" in mk
    for cite in ("mapper.py:256-263", "slam.py:126-127", "cameras.py:165-183", "tracker.py:399-401", "metric.py:181", "make_mesh.py:199",
                 "metric_obj.py:212", "csrc/map_repose.hip lists", "tests/repose_oracle.py restates them", "as exact bytes",
                 "keep their pose", "writes nothing and is counted", "every store is a 4-byte store"):
        assert cite in hdr, cite


def test_the_abi_did_not_move_and_the_structs_are_the_headers(native):
    hdr = _header()
    L = native.lib()
    assert L.dqo_abi_version() == 5 and "#define DQO_ABI_VERSION 5" in hdr
    assert L.dqo_abi_sizeof(17) == ctypes.sizeof(native.DqoWindowBank)
    assert L.dqo_abi_sizeof(18) == ctypes.sizeof(native.DqoTrajRepose) == 4 * 4 + 7 * 8
    assert L.dqo_abi_sizeof(19) == ctypes.sizeof(native.DqoReposeTarget) == 6 * 8 and L.dqo_abi_sizeof(20) == 0
    for st in (native.DqoTrajRepose, native.DqoReposeTarget):
        body = hdr[hdr.index("typedef struct %s {" % st.__name__):hdr.index("} %s;" % st.__name__)]
        names = re.findall(r"[*\s](\w+)(?=[,;])", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
        assert names == [n for n, _ in st._fields_], st.__name__
    assert list(native.REPOSE_TARGET_FIELDS) == [n for n, _ in native.DqoReposeTarget._fields_]
    assert "DQO_REPOSE_HAS_PROJMATRIX = 1" in hdr and native.REPOSE_HAS_PROJMATRIX == 1
    assert not [n for n in native.EXPORTS if "_bytes" in n and "repose" in n]  # no workspace


def _repose(native, **kw):
    f = dict(cap=8, n_new=8, T=3, flags=native.REPOSE_HAS_PROJMATRIX, pose=FAKE, header=FAKE + 4096, new_pose=FAKE + 8192,
             targets=FAKE + 12288, projection=FAKE + 16384, bank_state=None, stats=FAKE + 20480)
    f.update(kw)
    L = native.lib()
    rc = L.dqo_traj_repose(ctypes.byref(native.DqoTrajRepose(**f)), None)
    return rc, L.dqo_last_error().decode()


@pytest.mark.parametrize("case, kw, msg", [
    ("cap 0", dict(cap=0), "bad capacity"),
    ("cap negative", dict(cap=-4), "bad capacity"),
    ("null store", dict(pose=None), "null pointer"),
    ("null header", dict(header=None), "null pointer"),
    ("negative n_new", dict(n_new=-1), "bad n_new"),
    ("negative T", dict(T=-1), "bad target count"),
    ("targets without a table", dict(targets=None), "without a table"),
    ("projmatrix without projection", dict(projection=None), "projmatrix without a projection"),
])
def test_validation_before_launch(native, case, kw, msg):
    rc, err = _repose(native, **kw)
    assert rc == -1 and re.search(msg, err), (rc, err)


def test_null_arguments(native):
    L = native.lib()
    assert L.dqo_traj_repose(None, None) == -1 and b"null arguments" in L.dqo_last_error()


def test_the_source_is_one_launch_without_atomics_or_memset():
    src = open(os.path.join(ROOT, "dqo-map_amd", "csrc", "map_repose.hip")).read()
    code = "\n".join(l.split("//")[0] for l in src.splitlines())
    body = code[code.index("DQO_API int dqo_traj_repose("):]
    assert body[:body.index("\n}\n")].count("DQO_LAUNCH(") == 1
    assert "atomic" not in code and "hipMemset" not in code and "hipMemcpy" not in code and "Synchronize" not in code
    assert '#include "dqo_traj_camera.h"' in code and "#pragma clang fp contract(off)" in code
    traj = open(os.path.join(ROOT, "dqo-map_amd", "csrc", "map_traj.hip")).read()
    assert '#include "dqo_traj_camera.h"' in traj and "void traj_invert_affine" not in traj  # the statements live in one place
    shared = open(os.path.join(ROOT, "dqo-map_amd", "csrc", "dqo_traj_camera.h")).read()
    assert "void traj_invert_affine" in shared and "void traj_store_camera" in shared


def test_python_surface(native):
    import dqo_icp
    from dqo_harness import fused_mapping as F
    P = lambda f: [(n, p.default) for n, p in inspect.signature(f).parameters.items()]
    E = inspect.Parameter.empty
    assert P(dqo_icp.Trajectory.update_poses)[:3] == [("self", E), ("new_poses", E), ("targets", None)]
    assert P(dqo_icp.cameras_from_poses) == [("poses", E), ("projection", None), ("rows", None), ("out", None)]
    assert P(F.FusedMapper.update_poses) == [("self", E), ("traj", E), ("new_poses", None)]
    assert P(F.FusedMapper.set_frame)[-1] == ("row", None) and P(F.FusedMapper.bank_set)[-1] == ("row", None)
    assert P(F.FusedMapper.bank_set)[2:] == P(F.FusedMapper.set_frame)[2:]
    with pytest.raises(RuntimeError, match="GPU"):
        import torch
        dqo_icp.cameras_from_poses(torch.eye(4, dtype=torch.float64)[None])
