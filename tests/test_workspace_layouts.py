"""CPU: a workspace has one layout function, and its size is that function at a null base.  What holds it in place:

the sizes — tools/record_workspace_bytes.py's table of every size query over its grid (the steps where a part crosses an alignment or a
span) is, entry by entry, the table recorded from the commit before the layouts were unified (tests/workspace_bytes_parent.json): no
part moved, grew or changed its order; and the refusals — the entries whose one-byte-short workspace no other ABI test offers refuse it
with both numbers in the message, before anything is dereferenced or launched (the pointers are fakes)."""
import ctypes
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import record_workspace_bytes as rec  # noqa: E402


@pytest.fixture(scope="module")
def native():
    import __graft_entry__ as g
    g.build_hip()
    import _dqo_native
    return _dqo_native


@pytest.fixture(scope="module")
def tables(native):
    native.lib()  # (built and loadable)
    parent = json.load(open(os.path.join(ROOT, "tests", "workspace_bytes_parent.json")))
    return parent, rec.table(native.LIB_PATH)


def test_the_grid_names_every_size_query(tables):
    parent, now = tables
    assert sorted({k.split("(")[0] for k in now}) == rec.exports()
    assert sorted(parent) == sorted(now)


def test_every_size_is_the_parents(tables):
    parent, now = tables
    wrong = {k: (parent[k], now[k]) for k in parent if parent[k] != now[k]}
    assert not wrong, wrong


def test_invalid_arguments_still_give_zero(tables):
    _, now = tables
    bad = ([(f"dqo_mesh_{op}_workspace_bytes", a) for op in ("components", "smooth", "normals", "simplify", "cull") for a in rec.MESH_BAD]
           + [(q, a) for q in ("dqo_mesh_sample_workspace_bytes", "dqo_mesh_sample_counted_workspace_bytes") for a in rec.SAMPLE_BAD]
           + [("dqo_tsdf_workspace_bytes", a) for a in rec.TSDF_BAD]
           + [(q, a) for q in ("dqo_map_ssim_workspace_bytes", "dqo_growth_sample_workspace_bytes", "dqo_eval_picture_workspace_bytes",
                               "dqo_window_masks_workspace_bytes", "dqo_eval_ms_ssim_workspace_bytes", "dqo_eval_lpips_workspace_bytes")
              for a in rec.IMAGES_BAD[:3]]
           + [("dqo_eval_ms_ssim_workspace_bytes", (64, 48)), ("dqo_eval_lpips_workspace_bytes", (16, 16))]  # (below the smallest side)
           + [(q, a) for q in ("dqo_nn1_workspace_bytes", "dqo_nn1_grouped_workspace_bytes", "dqo_eval_pcd_workspace_bytes",
                               "dqo_eval_pcd_grouped_workspace_bytes") for a in ((-1, 1), (1, 1 << 25))])
    for query, args in bad:
        assert now[rec.key(query, args)] == 0, (query, args)


def _growth_sample(native, ws, ws_bytes):
    a = native.DqoGrowthSample()
    a.W, a.H, a.first_frame, a.uniform_sample_num, a.capacity, a.key_bits, a.M = 33, 17, 1, 10, 0, 32, 1
    a.vertex = a.normal = a.color = a.depth = a.header = 1
    a.workspace, a.workspace_bytes = ws, ws_bytes
    return native.lib().dqo_growth_sample(ctypes.byref(a), None)


# (the message's head, the size query and its sizes, the call given (native, ws, ws_bytes), the code): 1 stands for every required pointer
SHORT = [
    ("nn1 grouped", "dqo_nn1_grouped_workspace_bytes", (3, 4),
     lambda n, ws, b: n.lib().dqo_nn1_grouped(3, 1, 1, 4, 1, 1, None, None, 1, None, ws, b, None), -2),
    ("eval_pcd grouped", "dqo_eval_pcd_grouped_workspace_bytes", (3, 4),
     lambda n, ws, b: n.lib().dqo_eval_pcd_grouped(3, 1, 1, 4, 1, 1, None, 0, None, 1, 64, 0, ws, b, None), -2),
    ("growth sample", "dqo_growth_sample_workspace_bytes", (33, 17), _growth_sample, -2),
    # dqo_window_masks reports its workspace through its argument check: DQO_ERR_INVALID_ARG, as it always has
    ("window_masks", "dqo_window_masks_workspace_bytes", (33, 17),
     lambda n, ws, b: n.lib().dqo_window_masks(33, 17, 0, 1, None, None, 0.5, 0, 1, 1, 1, None, ws, b, None), -1),
    ("knn query", "dqo_knn3_query_workspace_bytes", (4, 5),
     lambda n, ws, b: n.lib().dqo_knn3_query_within(4, 1, 5, 1, 0.5, 1, 1, ws, b, None), -2),
    ("knn query", "dqo_knn3_query_workspace_bytes", (4, 5),
     lambda n, ws, b: n.lib().dqo_knn3_query_grouped(4, 1, 1, 5, 1, 1, None, 0.5, 1, 1, ws, b, None), -2),
]


@pytest.mark.parametrize("what,query,sizes,call,code", SHORT, ids=["nn1_grouped", "eval_pcd_grouped", "growth_sample", "window_masks",
                                                                   "knn3_query_within", "knn3_query_grouped"])
def test_a_workspace_one_byte_short_is_refused(native, what, query, sizes, call, code):
    lib = native.lib()
    need = getattr(lib, query)(*sizes)
    assert need > 0
    assert call(native, 1, need - 1) == code
    assert lib.dqo_last_error().decode() == f"{what} workspace too small ({need - 1} < {need})"
