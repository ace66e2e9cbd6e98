"""CPU-side checks of the keyframe bank's entry points (dqo_window_bank_arm, dqo_window_bank_select; csrc/map_window_bank.hip): the two
symbols are declared, exported and bound, the ABI did not move and no size query was added, the state's size and word order are the
header's, every argument error is reported before anything is dereferenced or launched (fake pointers; no GPU here), and the Python
surface is the documented one."""
import ctypes
import inspect
import os
import re

import pytest

import window_bank_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dqo_window_bank_arm", "dqo_window_bank_select")
FAKE = 0x10000  # a non-NULL address that is never dereferenced: every call below fails its checks before the launch


@pytest.fixture(scope="module")
def native():
    import __graft_entry__ as g
    g.build_hip()
    import _dqo_native
    return _dqo_native


def _header():
    return open(os.path.join(ROOT, "include", "dqo_raster.h")).read()


def test_symbols_are_declared_exported_and_bound(native):
    hdr = _header()
    lib = ctypes.CDLL(native.LIB_PATH)
    L = native.lib()
    for s in NEW:
        assert s + "(" in hdr and hasattr(lib, s) and s in native.EXPORTS
        assert getattr(L, s).argtypes
    assert L.dqo_window_bank_arm.argtypes == [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p]
    makefile = open(os.path.join(ROOT, "dqo-map_amd", "csrc", "Makefile")).read()
    assert "map_window_bank.hip" in makefile
    for cite in ("csrc/map_window_bank.hip lists", "tests/window_bank_oracle.py restates them", "iff  force != 0 or k != prev_k",
                 "iff  force != 0 or m != prev_m", "overrun = 1", "overrun = 2", "lost[lost_count] = c - 1", "the same grid on every call",
                 "Copies are exact bytes"):
        assert cite in hdr, cite


def test_the_abi_did_not_move_and_no_size_query_was_added(native):
    hdr = _header()
    L = native.lib()
    assert L.dqo_abi_version() == 5 and "#define DQO_ABI_VERSION 5" in hdr
    queries = re.findall(r"^size_t (dqo_\w+_bytes\w*)\(", hdr, flags=re.M)
    assert queries and not [q for q in queries if "bank" in q]
    assert not [n for n in native.EXPORTS if "_bytes" in n and "bank" in n]
    assert L.dqo_abi_sizeof(16) == 0 and L.dqo_abi_sizeof(17) == ctypes.sizeof(native.DqoWindowBank) == 4 * 4 + 21 * 8


def test_the_state_words_are_the_headers(native):
    hdr = _header()
    ticket = eval(re.search(r"#define DQO_TICKET_WORDS (\([^)]*\))", hdr).group(1))
    assert ticket == native.TICKET_WORDS == 16 + 16 * 64
    enum = dict(re.findall(r"(DQO_WINDOW_BANK_\w+) = DQO_TICKET_WORDS \+ (\d+)", hdr))
    assert int(enum.pop("DQO_WINDOW_BANK_STATE_WORDS")) + ticket == native.WINDOW_BANK_STATE_WORDS
    assert native.WINDOW_BANK_STATE_WORDS * 4 % 256 == 0  # padded as the other last-block heads are
    order = sorted(enum, key=lambda k: int(enum[k]))
    assert [k[len("DQO_WINDOW_BANK_"):].lower() for k in order] == list(native.WINDOW_BANK_WORDS) == list(O.WORDS)
    assert [int(enum[k]) for k in order] == list(range(len(O.WORDS)))
    # the struct of the header and the binding name the same fields in the same order
    body = hdr[hdr.index("typedef struct DqoWindowBank {"):hdr.index("} DqoWindowBank;")]
    names = re.findall(r"[*\s](\w+)(?=[,;])", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert names == [n for n, _ in native.DqoWindowBank._fields_]


def _select(native, **kw):
    f = dict(W=64, H=48, K_cap=3, n=8)
    for i, (name, _) in enumerate(native.DqoWindowBank._fields_[4:]):
        f[name] = FAKE + 4096 * i
    f.update(pixel_object=None, tile_objects=None, dst_pixel_object=None, dst_tile_objects=None)
    f.update(kw)
    lib = native.lib()
    rc = lib.dqo_window_bank_select(ctypes.byref(native.DqoWindowBank(**f)), None)
    return rc, lib.dqo_last_error().decode()


def test_validation_before_launch(native):
    lib = native.lib()
    assert lib.dqo_window_bank_arm(None, 4, None) == -1 and b"null state" in lib.dqo_last_error()
    assert lib.dqo_window_bank_arm(FAKE, -1, None) == -1 and b"bad schedule length" in lib.dqo_last_error()
    assert lib.dqo_window_bank_select(None, None) == -1 and b"null arguments" in lib.dqo_last_error()
    for k in (0, -2):
        rc, err = _select(native, K_cap=k)
        assert rc == -1 and "bad K_cap" in err, k
    for kw in (dict(W=0), dict(H=-1), dict(W=1 << 16, H=1 << 16)):
        rc, err = _select(native, **kw)
        assert rc == -1 and "bad image size" in err, kw
    rc, err = _select(native, n=-1)
    assert rc == -1 and "bad schedule length" in err
    for name in ("camera", "gt_color", "gt_depth", "render_mask", "tile_mask"):
        rc, err = _select(native, **{name: None})
        assert rc == -1 and "null bank part" in err, name
    for name in ("dst_bg", "dst_viewmatrix", "dst_projmatrix", "dst_campos", "dst_gt_color", "dst_gt_depth", "dst_render_mask", "dst_tile_mask"):
        rc, err = _select(native, **{name: None})
        assert rc == -1 and "null destination" in err, name
    for name in ("schedule", "state", "lost"):
        rc, err = _select(native, **{name: None})
        assert rc == -1 and "null schedule / state / lost" in err, name
    gate = dict(pixel_object=FAKE + 64, tile_objects=FAKE + 128, dst_pixel_object=FAKE + 192, dst_tile_objects=FAKE + 256)
    for name in gate:  # gate parts on one side only, or one of a pair
        rc, err = _select(native, **{k: v for k, v in gate.items() if k != name})
        assert rc == -1 and "the gate parts" in err, name
        rc, err = _select(native, **{name: gate[name]})
        assert rc == -1 and "the gate parts" in err, name
    rc, err = _select(native, pixel_object=gate["pixel_object"], tile_objects=gate["tile_objects"])
    assert rc == -1 and "the gate parts" in err


def test_the_source_uses_one_launch_and_no_other_atomics():
    src = open(os.path.join(ROOT, "dqo-map_amd", "csrc", "map_window_bank.hip")).read()
    code = "\n".join(l.split("//")[0] for l in src.splitlines())
    for name in NEW:
        body = code[code.index(f"DQO_API int {name}("):]
        assert body[:body.index("\n}\n")].count("DQO_LAUNCH(") == 1, name
    assert "dqo_last_block(" in code and "atomicAdd" not in code and "atomicExch" not in code and "atomicCAS" not in code
    assert "hipMemset" not in code and "hipMemcpy" not in code and "Synchronize" not in code
    assert not re.search(r"\b(float|double)\b(?!\s*\*)", code.replace("const float*", "").replace("float *", ""))  # no float arithmetic


def test_python_surface(native):
    from dqo_harness import fused_mapping as F
    from dqo_harness import map_operators as M
    P = lambda f: [(n, p.default) for n, p in inspect.signature(f).parameters.items()]
    E = inspect.Parameter.empty
    assert P(F.FusedMapper.run_bank) == [("self", E), ("schedule", E), ("check_every", 64), ("capacity_margin", 1.5)]
    assert P(F.FusedMapper.run_bank)[1:] == P(F.FusedMapper.run_window)[1:]
    assert P(F.FusedMapper.bank_set)[2:] == P(F.FusedMapper.set_frame)[2:]
    assert P(M.MapOperators.refresh_bank)[2:] == P(M.MapOperators.refresh_window)[2:]
    assert "refresh_bank" in vars(M.MapOperators) and "capture_bank" in vars(F.FusedMapper)
    sig = inspect.signature(F.FusedMapper.capture_bank).parameters
    assert list(sig)[:3] == ["self", "frames", "slots"] and sig["slots"].default is None and sig["unroll"].default == 1
    assert inspect.signature(F.FusedMapper.capture).parameters["head"].default is None  # today's behaviour unless a bank asks
    fm = F.FusedMapper.__new__(F.FusedMapper)
    fm._bank = None
    for call in (lambda: fm.run_bank([0]), lambda: fm.bank_set(0), lambda: fm._require_bank("refresh_bank")):
        with pytest.raises(RuntimeError, match="no keyframe bank"):
            call()
    fm.attach_count_reducer = lambda n: n  # a shard
    with pytest.raises(NotImplementedError, match="sharded mapper"):
        fm.capture_bank([dict()])
    with pytest.raises(NotImplementedError, match="sharded mapper"):
        fm.refresh_bank()
    fm.attach_count_reducer = None
    with pytest.raises(RuntimeError, match="per-frame choice"):
        fm.capture_bank([dict()], list_split="auto")
