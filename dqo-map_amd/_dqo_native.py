"""ctypes binding of libdqoraster.so.  Shared by the drop-in packages in this directory.

The structs, the entry points with their argument and return types, and the constants are read from include/dqo_raster.h
(_dqo_header.py states the rules): a new operator adds its declaration to the header and nothing here, except that a new struct adds its
name to ABI_SIZEOF_ORDER.

There is NO CPU fallback: if the HIP library is missing or a tensor is not on the GPU the call raises.
"""
import ctypes
import os

import _dqo_header

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libdqoraster.so")

_HEADER = _dqo_header.load()
CONSTANTS = _HEADER.constants    # {"DQO_X": int}: every #define and enumerator of the header
PROTOTYPES = _HEADER.functions   # {"dqo_name": (restype, [argtypes])}
EXPORTS = tuple(PROTOTYPES)
# the struct classes (DqoRastParams, ...): callers and CPU tests construct them without the library
globals().update({name: type(name, (ctypes.Structure,), {"_fields_": fields}) for name, fields in _HEADER.structs.items()})

ROW_FROZEN, ROW_HIDDEN = CONSTANTS["DQO_ROW_FROZEN"], CONSTANTS["DQO_ROW_HIDDEN"]
# a DqoReposeTarget as the columns of an int64 [T,6] device table
REPOSE_TARGET_FIELDS = tuple(n for n, _ in _HEADER.structs["DqoReposeTarget"])
REPOSE_HAS_PROJMATRIX = CONSTANTS["DQO_REPOSE_HAS_PROJMATRIX"]
TICKET_WORDS = CONSTANTS["DQO_TICKET_WORDS"]
# the state words of the keyframe bank behind its ticket, in order, and the state's size
WINDOW_BANK_STATE_WORDS = CONSTANTS["DQO_WINDOW_BANK_STATE_WORDS"]
WINDOW_BANK_WORDS = tuple(k[len("DQO_WINDOW_BANK_"):].lower() for k in sorted(CONSTANTS, key=CONSTANTS.get)
                          if k.startswith("DQO_WINDOW_BANK_") and CONSTANTS[k] < WINDOW_BANK_STATE_WORDS)

# dqo_abi_sizeof's index -> struct.  csrc/dqo_capi.hip defines this order, not the header: the one hand-kept list (None: unused index)
ABI_SIZEOF_ORDER = ("DqoRastParams", "DqoRastInputs", "DqoRastOutputs", "DqoRastCtx", "DqoRastGrads", "DqoRastHeader", "DqoProfileEntry",
                    "DqoAdamStep", "DqoLossTap", "DqoObjectGate", "DqoAdamTensor", "DqoRastParamInputs", "DqoRastParamGrads", None,
                    "DqoLifecycle", "DqoGrowthSample", None, "DqoWindowBank", "DqoTrajRepose", "DqoReposeTarget")

_lib = None


def lib():
    """Load libdqoraster.so (built by `make -C dqo-map_amd/csrc` / __graft_entry__.build()).  Fails loudly when absent."""
    global _lib
    if _lib is None:
        # torch first: it loads its bundled HIP runtime; libdqoraster.so then binds to that same copy (same SONAME).  The
        # other order puts two ROCr instances in one process and the second one sees "no ROCm-capable device".
        import torch  # noqa: F401
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} not found: the HIP extension is not built (run __graft_entry__.build()). "
                               "There is no CPU fallback for this operator.")
        L = ctypes.CDLL(LIB_PATH)
        for name, (restype, argtypes) in PROTOTYPES.items():  # (ctypes' default restype, c_int, would cut a size_t at 2 GiB)
            fn = getattr(L, name)
            fn.restype, fn.argtypes = restype, argtypes
        if L.dqo_abi_version() != CONSTANTS["DQO_ABI_VERSION"]:
            raise RuntimeError("libdqoraster.so ABI version mismatch")
        for k, name in enumerate(ABI_SIZEOF_ORDER):
            if name is not None and L.dqo_abi_sizeof(k) != ctypes.sizeof(globals()[name]):
                raise RuntimeError(f"libdqoraster.so: struct {name} is {L.dqo_abi_sizeof(k)} bytes in the library, "
                                   f"{ctypes.sizeof(globals()[name])} in the binding")
        _lib = L
    return _lib


def check(rc):
    if rc != 0:
        raise RuntimeError(lib().dqo_last_error().decode() or f"libdqoraster error {rc}")


def ptr(t):
    """Raw device pointer of a torch tensor (None / empty tensor -> NULL, like an empty tensor's data_ptr in the reference)."""
    if t is None or t.numel() == 0:
        return None
    return t.data_ptr()


def require_gpu(*tensors):
    for t in tensors:
        if t is not None and t.numel() > 0 and not t.is_cuda:
            raise RuntimeError("libdqoraster operators need GPU (ROCm) tensors; there is no CPU path. Got a tensor on "
                               f"{t.device}.")


def require_gpu_op(principal, *others):
    """The device rule of an operator's wrapper.  `principal` (a tensor, or a tuple of tensors) names the device the call runs on: it
    must be a GPU tensor even when it is empty.  `others` (None allowed) follow require_gpu's rule: an empty one may live anywhere."""
    principal = principal if isinstance(principal, tuple) else (principal,)
    require_gpu(*principal, *others)
    if not all(t.is_cuda for t in principal):
        raise RuntimeError("libdqoraster operators need GPU (ROCm) tensors; there is no CPU path.")


def current_stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def profile_enable(on):
    lib().dqo_profile_enable(1 if on else 0)


def profile_collect(reset=True):
    """{kernel name: (total_ms, calls)} of every launch bracketed since the last reset (synchronises)."""
    buf = (DqoProfileEntry * 64)()  # noqa: F821 (a struct class of the header)
    n = lib().dqo_profile_collect(buf, 64, 1 if reset else 0)
    return {buf[i].name.decode(): (buf[i].total_ms, buf[i].calls) for i in range(n)}
