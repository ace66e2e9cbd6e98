"""CPU-side checks of the object stage's entry points (include/dqo_raster.h: dqo_objmap_frame / dqo_objmap_optimize / dqo_objmap_mean_iou;
dqo_quadrics.ObjectMap): the symbols are declared, exported and bound, and every argument error is reported before anything is launched
(no GPU here)."""
import ctypes
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dqo_objmap_frame", "dqo_objmap_optimize", "dqo_objmap_mean_iou")
FAKE = 0x10000  # a non-NULL address that is never dereferenced: every call below fails its checks before any launch
TABLE = ("axes", "R", "center", "cat", "uid", "nviews", "view_P34", "view_bbox", "state")
FRAME_IN = ("bbox", "ellipse", "det_cat", "score", "depth", "K", "Rt")
FRAME_OUT = ("fate", "row", "det_depth", "opt_flag", "header")


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
        assert getattr(native.lib(), s).argtypes is not None
    assert native.lib().dqo_abi_version() == 5
    for cite in ("mapper.py:147-165", "mapper.py:204-205", "mapper.py:1512-1531", "quadrics.py:336-386", ":429-538", ":926-968", ":1013-1217",
                 ":2397-2425", "quadrics.py:2234-2298"):
        assert cite in hdr, cite  # the reference lines they replace
    src = open(os.path.join(ROOT, "dqo-map_amd", "csrc", "Makefile")).read()
    assert "map_objects.hip" in src and re.search(r"map_objects\.o: HIPFLAGS \+= -ffp-contract=off", src)


def _frame(native, **kw):
    a = dict(cap_obj=256, cap_views=64, cap_det=64, M=8, W=160, H=120, frame_id=3, seed=5)
    a.update({k: FAKE for k in TABLE + FRAME_IN + FRAME_OUT})
    a.update(kw)
    L = native.lib()
    rc = L.dqo_objmap_frame(a["cap_obj"], a["cap_views"], a["cap_det"], *[a[k] for k in TABLE], a["M"], *[a[k] for k in FRAME_IN], a["W"], a["H"],
                            a["frame_id"], a["seed"], *[a[k] for k in FRAME_OUT], None)
    return rc, L.dqo_last_error().decode()


@pytest.mark.parametrize("kw, msg", [(dict(cap_obj=0), "bad capacities"), (dict(cap_obj=1025), "bad capacities"), (dict(cap_obj=-1), "bad capacities"),
                                      (dict(cap_views=1), "bad capacities"), (dict(cap_obj=1024, cap_views=1 << 20), "bad capacities"),
                                      (dict(cap_det=0), "cap_det"), (dict(cap_det=65), "cap_det"), (dict(M=0), "bad detection count"),
                                      (dict(M=-2), "bad detection count"), (dict(M=65), "bad detection count"),
                                      (dict(cap_det=8, M=9), "bad detection count 9: 1 to cap_det = 8"), (dict(W=0), "bad image size"),
                                      (dict(H=-1), "bad image size"), (dict(W=1 << 20, H=1 << 20), "bad image size")] +
                         [({k: None}, "null pointer") for k in TABLE + FRAME_IN + FRAME_OUT])
def test_frame_validation_errors_without_a_gpu(native, kw, msg):
    rc, err = _frame(native, **kw)
    assert rc == -1 and re.search(msg, err), (rc, err)  # DQO_ERR_INVALID_ARG


OPT = ("axes", "R", "center", "uid", "nviews", "view_P34", "view_bbox", "state", "opt_flag")
IOU = ("axes", "R", "center", "nviews", "view_P34", "view_bbox", "state", "mean_iou")


def _optimize(native, **kw):
    a = dict(cap_obj=256, cap_views=64, frame_id=3, seed=5, loss_hist=None)
    a.update({k: FAKE for k in OPT})
    a.update(kw)
    L = native.lib()
    rc = L.dqo_objmap_optimize(a["cap_obj"], a["cap_views"], *[a[k] for k in OPT], a["frame_id"], a["seed"], a["loss_hist"], None)
    return rc, L.dqo_last_error().decode()


def _mean_iou(native, **kw):
    a = dict(cap_obj=256, cap_views=64)
    a.update({k: FAKE for k in IOU})
    a.update(kw)
    L = native.lib()
    rc = L.dqo_objmap_mean_iou(a["cap_obj"], a["cap_views"], *[a[k] for k in IOU], None)
    return rc, L.dqo_last_error().decode()


@pytest.mark.parametrize("kw, msg", [(dict(cap_obj=0), "bad capacities"), (dict(cap_obj=1025), "bad capacities"), (dict(cap_views=1), "bad capacities")] +
                         [({k: None}, "null pointer") for k in OPT])
def test_optimize_validation_errors_without_a_gpu(native, kw, msg):
    rc, err = _optimize(native, **kw)
    assert rc == -1 and re.search(msg, err), (rc, err)


@pytest.mark.parametrize("kw, msg", [(dict(cap_obj=0), "bad capacities"), (dict(cap_obj=1025), "bad capacities"), (dict(cap_views=0), "bad capacities")] +
                         [({k: None}, "null pointer") for k in IOU])
def test_mean_iou_validation_errors_without_a_gpu(native, kw, msg):
    rc, err = _mean_iou(native, **kw)
    assert rc == -1 and re.search(msg, err), (rc, err)


def test_python_entry(native):
    import dqo_quadrics as dq
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(dq.ObjectMap.__init__) == ["self", "cap_obj", "cap_views", "cap_det", "device"]
    assert [inspect.signature(dq.ObjectMap.__init__).parameters[k].default for k in ("cap_obj", "cap_views", "cap_det")] == [256, 64, 64]
    assert sig(dq.ObjectMap.frame) == ["self", "dets", "depth", "K", "Rt", "frame_id", "seed"]
    assert sig(dq.ObjectMap.optimize)[:3] == ["self", "frame_id", "seed"]
    for m in ("mean_iou", "view_csr", "to_host", "state_dict", "load_state_dict"):
        assert callable(getattr(dq.ObjectMap, m))
    assert dq.FATES == ("dropped", "invalidated", "matched", "new", "replaced", "unmatched") and len(dq.FRAME_HEADER) == 8
    with pytest.raises(RuntimeError, match="GPU"):
        dq.ObjectMap(device="cpu")


def test_oracle_and_binding_agree_on_the_enumerations():
    import dqo_quadrics as dq
    import object_oracle as O
    assert O.FATES == dq.FATES and O.HEADER == dq.FRAME_HEADER
