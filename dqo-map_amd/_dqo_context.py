"""The rasteriser context on the Python side: its three byte buffers, their sizing rules and the frame header at the head of `geom`.

The C side owns the layouts (dqo_*_layout, check_common / check_render, dqo_rast_read_header: csrc/dqo_capi.hip); this module is their one
Python counterpart.  The drop-in op (diff_gaussian_rasterization_depth) and dqo_harness.FusedMapper get their buffers, their DqoRastCtx
structs, their capacities and every header word from here.  No caching, no pool, no modes: those belong to the callers.
"""
import ctypes

import torch

import _dqo_native as N

_WORD = {name: i for i, (name, _) in enumerate(N.DqoRastHeader._fields_)}  # word index of every DqoRastHeader field
HEADER_KEYS = tuple(n for n in _WORD if n not in ("stage", "reserved"))


def header_dict(words):
    """The frame header as a dict (num_rendered = instances kept in the tile lists, num_candidates = the reference's num_rendered,
    num_tiles, max_tile_count, num_visible, overflow) from its eight int32 words: a list, a host tensor or a DqoRastHeader."""
    if isinstance(words, N.DqoRastHeader):
        return {k: int(getattr(words, k)) for k in HEADER_KEYS}
    if torch.is_tensor(words):
        words = words.tolist()
    return {k: words[_WORD[k]] for k in HEADER_KEYS}


def header_words(geom):
    """The header's eight int32 words at the head of geometry buffer `geom`, as a view in device memory."""
    return geom[:ctypes.sizeof(N.DqoRastHeader)].view(torch.int32)


def read_header(geom):
    """The header of the frame last rendered on `geom`: one 32-byte device-to-host read (synchronises)."""
    return header_dict(header_words(geom).cpu())


def overflowed(geom):
    """Whether the frame last rendered on `geom` outgrew its context: one 4-byte device-to-host read (synchronises)."""
    at = 4 * _WORD["overflow"]
    return bool(geom[at:at + 4].view(torch.int32).item())


def bucket_for(longest, short_margin=1.3):
    """Per-tile list bucket (DqoRastCtx.tile_bucket_capacity) for lists of up to `longest` entries: a power of two, at least twice that;
    1024 instead of 2048 while short_margin x longest still fits — 1024 entries are what the per-tile sort launch reaches, so the
    long-list sort launch disappears (pass 2.0 to never trade margin for that launch).  A tile that outgrows its bucket raises the same
    overflow flag as running out of instance capacity."""
    b = 256
    while b < 2 * longest:
        b *= 2
    if b == 2048 and short_margin * longest <= 1024:
        b = 1024
    return b


def capacity_for(count, margin):
    """Instance capacity for a frame that was measured at `count` (Gaussian, tile) pairs, with room for the map to move."""
    return int(count * margin) + 4096


def forward_call(stage, params, inputs, outputs, cctx, *rest, pinputs=None):
    """dqo_rast_forward_<stage> of the activated form, or its _params counterpart when the parameter form's inputs are given."""
    b = ctypes.byref
    if pinputs is None:
        return N.check(getattr(N.lib(), "dqo_rast_forward" + stage)(b(params), b(inputs), b(outputs), b(cctx), *rest))
    return N.check(getattr(N.lib(), "dqo_rast_forward" + stage + "_params")(b(params), b(inputs), b(pinputs), b(outputs), b(cctx), *rest))


class RastContext:
    """The context buffers of one (P, W, H): geom and img from construction, binning once size() knows the instance capacity `cap` and
    the per-tile bucket (0: packed lists)."""
    __slots__ = ("geom", "img", "binning", "cap", "bucket", "P", "W", "H")

    def __init__(self, P, W, H, device):
        lib, u8 = N.lib(), dict(dtype=torch.uint8, device=device)
        self.P, self.W, self.H = P, W, H
        self.geom = torch.empty((lib.dqo_rast_geom_bytes(P, W, H),), **u8)
        self.img = torch.empty((lib.dqo_rast_image_bytes(W, H),), **u8)
        self.binning, self.cap, self.bucket = None, 0, 0

    @classmethod
    def over(cls, P, W, H, geom, img, binning, cap, bucket=0):
        """The context a forward left behind, over its buffers (the backward's saved tensors)."""
        self = cls.__new__(cls)
        self.P, self.W, self.H, self.geom, self.img, self.binning, self.cap, self.bucket = P, W, H, geom, img, binning, cap, bucket
        return self

    def size(self, cap, bucket=0):
        self.cap, self.bucket = cap, bucket
        self.binning = torch.empty((N.lib().dqo_rast_binning_bytes_bucketed(cap, self.W, self.H, bucket),), dtype=torch.uint8,
                                   device=self.geom.device)
        return self

    def cctx(self, **fields):
        """A new DqoRastCtx over the buffers; fields: the per-call members (list_split, keep_tile_order, frame_prezeroed, loss_tap,
        object_gate — the structs the two pointers name are the caller's to keep alive)."""
        b = self.binning
        return N.DqoRastCtx(geom=self.geom.data_ptr(), geom_bytes=self.geom.numel(), binning=None if b is None else b.data_ptr(),
                            binning_bytes=0 if b is None else b.numel(), image=self.img.data_ptr(), image_bytes=self.img.numel(),
                            inst_capacity=self.cap, tile_bucket_capacity=self.bucket, **fields)

    def header(self, stream):
        """dqo_rast_read_header: the DqoRastHeader of the stage that ran last on `stream` (synchronises it; raises if the frame
        overflowed).  After stage 1 only num_visible and num_candidates are known."""
        hdr = N.DqoRastHeader()
        N.check(N.lib().dqo_rast_read_header(ctypes.byref(self.cctx()), ctypes.byref(hdr), stream))
        return hdr

    def measure(self, params, inputs, outputs, stream, pinputs=None, **fields):
        """Stage 1 and the one header read behind it: num_candidates (the reference's num_rendered, an upper bound of the instances
        the binning keeps) sizes the binning buffer, num_visible counts the Gaussians in view."""
        forward_call("_prepare", params, inputs, outputs, self.cctx(**fields), stream, pinputs=pinputs)
        return self.header(stream)

    def render(self, params, inputs, outputs, stream, pinputs=None, prepare=False, **fields):
        """Stage 2 of a measured frame on the sized context; prepare: both stages in one call (dqo_rast_forward, activated form only)."""
        forward_call("" if prepare else "_render", params, inputs, outputs, self.cctx(**fields), stream, pinputs=pinputs)
