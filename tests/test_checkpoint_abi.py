"""CPU-side checks of the map checkpoint (include/dqo_raster.h: dqo_map_pack_rows / dqo_map_unpack_rows; dqo_ply's vertex table): the
symbols are declared and exported, every argument error is reported before anything is launched (no GPU here), and
write_vertex_table / read_vertex_table are save_model_ply's file, byte for byte, and its inverse."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from checkpoint_cases import hand_table, values

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dqo_map_pack_workspace_bytes", "dqo_map_pack_rows", "dqo_map_unpack_rows")
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
    assert "mapper.py:1571-1608" in hdr and "gaussian_pointcloud.py:132-207" in hdr  # the reference lines they replace


def _pack(native, **kw):
    a = dict(P=1000, M=16, conf=1, xyz=FAKE, shs=FAKE, opacity=FAKE, scaling=FAKE, rotation=FAKE, confidence=None, alive=None, stable=None,
             table=FAKE, table_rows=1000, header=FAKE, ws=FAKE, ws_bytes=1 << 40)
    a.update(kw)
    L = native.lib()
    rc = L.dqo_map_pack_rows(a["P"], a["M"], a["conf"], a["xyz"], a["shs"], a["opacity"], a["scaling"], a["rotation"], a["confidence"],
                             a["alive"], a["stable"], a["table"], a["table_rows"], a["header"], a["ws"], a["ws_bytes"], None)
    return rc, L.dqo_last_error().decode()


def _unpack(native, **kw):
    a = dict(P=1000, M=16, n=10, first_row=0, conf=1, table=FAKE, xyz=FAKE, shs=FAKE, opacity=FAKE, scaling=FAKE, rotation=FAKE, confidence=FAKE)
    a.update(kw)
    L = native.lib()
    rc = L.dqo_map_unpack_rows(a["P"], a["M"], a["n"], a["first_row"], a["conf"], a["table"], a["xyz"], a["shs"], a["opacity"], a["scaling"],
                               a["rotation"], a["confidence"], None)
    return rc, L.dqo_last_error().decode()


@pytest.mark.parametrize("case, kw, msg", [
    ("P 0", dict(P=0, table_rows=0), "bad row count"),
    ("P negative", dict(P=-3), "bad row count"),
    ("M 0", dict(M=0), "bad SH size"),
    ("M negative", dict(M=-1), "bad SH size"),
    ("M 65", dict(M=65), "bad SH size"),
    ("2^31 floats", dict(P=(1 << 31) // 63 + 1, table_rows=1 << 40), "2\\^31 - 1 floats"),
    ("null xyz", dict(xyz=None), "null pointer"),
    ("null shs", dict(shs=None), "null pointer"),
    ("null opacity", dict(opacity=None), "null pointer"),
    ("null scaling", dict(scaling=None), "null pointer"),
    ("null rotation", dict(rotation=None), "null pointer"),
    ("null table", dict(table=None), "null pointer"),
    ("null header", dict(header=None), "null pointer"),
    ("short table", dict(table_rows=999), "table capacity 999 rows"),
])
def test_pack_validation_errors_without_a_gpu(native, case, kw, msg):
    rc, err = _pack(native, **kw)
    assert rc == -1 and re.search(msg, err), (rc, err)  # DQO_ERR_INVALID_ARG


def test_pack_short_or_missing_workspace(native):
    L = native.lib()
    need = L.dqo_map_pack_workspace_bytes(1000)
    assert need > 0
    for kw in (dict(ws_bytes=need - 1), dict(ws=None)):
        rc, err = _pack(native, **kw)
        assert rc == -2 and "workspace" in err, (rc, err)  # DQO_ERR_WORKSPACE
    # (the largest table: 2^31 - 1 floats exactly passes the size check and then fails on its workspace)
    rc, err = _pack(native, P=(1 << 31) // 63, table_rows=1 << 40, ws_bytes=16)
    assert (1 << 31) // 63 * 63 <= (1 << 31) - 1 and rc == -2, (rc, err)


def test_pack_workspace_bytes(native):
    f = native.lib().dqo_map_pack_workspace_bytes
    assert f(0) == 0 and f(-1) == 0
    assert 0 < f(1) <= f(256) < f(2000000) and f(1) % 256 == 0
    assert f(2000000) >= 4352 + 8 * ((2000000 + 255) // 256)  # the ticket words, then one pair per block of 256 rows


@pytest.mark.parametrize("case, kw, msg", [
    ("P 0", dict(P=0, n=0), "bad size"),
    ("n negative", dict(n=-1), "bad size"),
    ("first_row negative", dict(first_row=-1), "bad size"),
    ("past the end", dict(first_row=995, n=6), "bad size"),
    ("past int32", dict(P=(1 << 31) - 1, first_row=(1 << 31) - 2, n=(1 << 31) - 2), "bad size"),
    ("M 0", dict(M=0), "bad SH size"),
    ("M 65", dict(M=65), "bad SH size"),
    ("2^31 floats", dict(P=(1 << 31) // 63 + 1), "2\\^31 - 1 floats"),
    ("null table", dict(table=None), "null pointer"),
    ("null xyz", dict(xyz=None), "null pointer"),
    ("null shs", dict(shs=None), "null pointer"),
    ("null opacity", dict(opacity=None), "null pointer"),
    ("null scaling", dict(scaling=None), "null pointer"),
    ("null rotation", dict(rotation=None), "null pointer"),
])
def test_unpack_validation_errors_without_a_gpu(native, case, kw, msg):
    rc, err = _unpack(native, **kw)
    assert rc == -1 and re.search(msg, err), (rc, err)


def test_unpack_of_no_rows_does_nothing(native):
    assert _unpack(native, n=0, table=None)[0] == 0


@pytest.mark.parametrize("M", [1, 16])
@pytest.mark.parametrize("include_confidence", [True, False])
def test_write_vertex_table_is_save_model_ply_and_read_inverts_it(native, tmp_path, M, include_confidence):
    import dqo_ply
    v = values(37, M, 5 + M)
    want, got = str(tmp_path / "want.ply"), str(tmp_path / "got.ply")
    dqo_ply.save_model_ply(want, v["xyz"], v["shs"], v["opacity_raw"], v["scaling_raw"], v["rotation_raw"], v["confidence"],
                           include_confidence=include_confidence)
    table = hand_table(v, include_confidence)
    assert dqo_ply.write_vertex_table(got, table, 3 * (M - 1), include_confidence) == 37
    assert open(got, "rb").read() == open(want, "rb").read()
    names, back = dqo_ply.read_vertex_table(got)
    assert names == dqo_ply.attribute_names(3 * (M - 1), include_confidence)
    assert back.dtype == np.float32 and back.view(np.uint32).tobytes() == table.view(np.uint32).tobytes()
    # a slice of a larger table (what save_model writes its files from) and a host tensor
    import torch
    big = np.concatenate([table, table[::-1]])
    assert dqo_ply.write_vertex_table(got, torch.from_numpy(big)[:37], 3 * (M - 1), include_confidence) == 37
    assert open(got, "rb").read() == open(want, "rb").read()
    # and load_model_ply reads the same values back
    d = dqo_ply.load_model_ply(got, max_sh_degree=int(round(M ** 0.5)) - 1)
    for k in ("xyz", "shs", "scaling_raw", "rotation_raw", "opacity_raw"):
        assert np.ascontiguousarray(d[k]).view(np.uint32).tobytes() == v[k].view(np.uint32).tobytes(), k
    conf = v["confidence"] if include_confidence else np.zeros((37, 1), np.float32)
    assert np.ascontiguousarray(d["confidence"]).view(np.uint32).tobytes() == conf.view(np.uint32).tobytes()


def test_zero_rows_write_no_file_and_bad_tables_are_refused(native, tmp_path):
    import dqo_ply
    p = str(tmp_path / "none.ply")
    assert dqo_ply.write_vertex_table(p, np.zeros((0, 63), np.float32), 45, True) == 0 and not os.path.exists(p)
    for bad in (np.zeros((3, 62), np.float32), np.zeros((3, 63), np.float64), np.zeros((3, 126), np.float32)[:, ::2], np.zeros((63,), np.float32)):
        with pytest.raises(ValueError, match="write_vertex_table"):
            dqo_ply.write_vertex_table(p, bad, 45, True)
    assert not os.path.exists(p)


def test_python_entry(native):
    import torch
    import dqo_ply
    from dqo_harness.fused_mapping import FusedMapper
    assert list(inspect.signature(dqo_ply.write_vertex_table).parameters) == ["path", "table", "n_rest", "include_confidence"]
    assert list(inspect.signature(dqo_ply.read_vertex_table).parameters) == ["path"]
    assert list(inspect.signature(FusedMapper.pack_rows).parameters) == ["self", "include_confidence", "out"]
    assert list(inspect.signature(FusedMapper.save_model).parameters) == ["self", "path", "save_data", "save_sibr", "save_merge"]
    assert list(inspect.signature(FusedMapper.load_model).parameters) == ["self", "path", "stable_path", "tick"]
    assert list(inspect.signature(FusedMapper.from_model_ply).parameters) == ["path", "stable_path", "settings", "device", "spare_rows", "kw"]
    z = lambda *s: torch.zeros(*s)
    with pytest.raises(RuntimeError, match="GPU"):
        dqo_ply.pack_rows(z(4, 3), z(4, 1, 3), z(4, 1), z(4, 3), z(4, 4))
    with pytest.raises(RuntimeError, match="GPU"):
        dqo_ply.unpack_rows(z(2, 17), 0, z(4, 3), z(4, 1, 3), z(4, 1), z(4, 3), z(4, 4))
