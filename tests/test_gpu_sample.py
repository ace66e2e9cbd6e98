"""GPU: the growth sampler (dqo_mapgrowth.temp_points_init, FusedMapper.sample_new — csrc/map_sample.hip) against the numpy oracle
(tests/sample_oracle.py, itself held to torch on the reference's statements by tests/test_sample_oracle.py).  EQUAL: the header integers,
the chosen pixels and their order, xyz, shs, scales, opacity, obj_id and the normalised normal, bit for bit.  Rotations of the compute_rot
path: the statements up to the arguments of acos / sin / cos are the oracle's own IEEE statements on the bit-equal normal; the three
library functions get 4 x the distance measured on the CPU between torch's float32 results and the same functions in double on the same
arguments over the fixture's rows — 1.1920928955078125e-07 (test_sample_oracle.py::test_the_rotation_bar_is_measured,
profiles/r08_sample_rotation_bar.txt), so the bar is 4.76837158203125e-07."""
import functools

import numpy as np
import pytest

import sample_cases as sc
from sample_oracle import rotations, sample_keys, sample_oracle

pytestmark = pytest.mark.gpu

ROTATION_BAR = 4 * 1.1920928955078125e-07
EXACT = ("pixel", "xyz", "normal", "shs", "scales", "opacity", "obj_id")


def _cuda(d):
    import torch
    return None if d is None else {k: None if v is None else torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in d.items()}


def _run(frame, model, **kw):
    import torch
    import dqo_mapgrowth as mg
    new, header = mg.temp_points_init(_cuda(frame), _cuda(model), tick=4, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in new.items()}, header


def _bits(x):
    return np.ascontiguousarray(x).view(np.int32) if x.dtype == np.float32 else x


def _assert_rows(got, header, want, identity):
    for k, v in want["header"].items():
        assert header[k] == v, (k, header, want["header"])
    assert header["tick"] == 4
    for k in EXACT:
        if want[k] is None:
            assert k not in got
            continue
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, (k, got[k].shape, want[k].shape)
        assert np.array_equal(_bits(got[k]), _bits(want[k])), (k, np.nonzero((_bits(got[k]) != _bits(want[k])).reshape(len(want[k]), -1).any(1))[0][:8])
    if identity:
        assert np.array_equal(_bits(got["rotations"]), _bits(want["rotations"]))
    elif len(want["rotations"]):
        d = float(np.abs(got["rotations"].astype(np.float64) - want["rotations"]).max())
        print("rotation distance to the oracle:", d, "bar:", ROTATION_BAR)
        assert d <= ROTATION_BAR


@pytest.mark.parametrize("xyz_factor", [(1.0, 1.0, 1.0), (1.0, 1.0, 0.1)], ids=["identity", "compute_rot"])
@pytest.mark.parametrize("instance", [True, False], ids=["instance", "plain"])
@pytest.mark.parametrize("first", [True, False], ids=["first", "later"])
def test_a_small_frame_equals_the_oracle(first, instance, xyz_factor):
    """50 x 36: four blocks of 512 pixels, the last one partial; every kind of pixel (tests/sample_cases.py)."""
    frame, model = sc.make_frame(instance=instance)
    kw = dict(sc.SMALL, xyz_factor=xyz_factor, seed=11)
    want = sample_oracle(frame, None if first else model, **kw)
    assert want["header"]["k_a"] > 0 and (first or want["header"]["k_b"] > 0) and want["header"]["rows"] < want["header"]["k_a"] + want["header"]["k_b"]
    got, header = _run(frame, None if first else model, **kw)
    _assert_rows(got, header, want, xyz_factor == (1.0, 1.0, 1.0))


DEGENERATE = {
    "empty_mask": (lambda: sc.blank_frame(36, 50, []), dict(sc.SMALL), True),
    "k_zero": (lambda: sc.make_frame(), dict(sc.SMALL, transmission_sample_ratio=1e-4, error_sample_ratio=1e-4), False),
    "k_trans_zero_only": (lambda: sc.make_frame(), dict(sc.SMALL, transmission_sample_ratio=1e-4), False),
    "k_clamped": (lambda: sc.make_frame(), dict(sc.SMALL, uniform_sample_num=10 ** 6, error_sample_ratio=1.0), False),
    "first_k_clamped": (lambda: sc.make_frame(), dict(sc.SMALL, uniform_sample_num=10 ** 6), True),
    "one_pixel": (lambda: sc.blank_frame(36, 50, [1234]), dict(sc.SMALL), True),
    "one_whole_block": (lambda: sc.blank_frame(36, 50, np.arange(512, 1024)), dict(sc.SMALL, uniform_sample_num=100), True),
}


@pytest.mark.parametrize("name", list(DEGENERATE))
def test_degenerate_masks_and_counts(name):
    make, kw, first = DEGENERATE[name]
    frame, model = make()
    kw = dict(kw, seed=5)
    want = sample_oracle(frame, None if first else model, **kw)
    h = want["header"]
    expect = dict(empty_mask=h["rows"] == 0 and h["mask_a"] == 0, k_zero=h["k_a"] == 0 and h["k_b"] == 0 and h["rows"] == 0 and h["mask_b"] > 0,
                  k_trans_zero_only=h["k_a"] == 0 and h["k_b"] > 0, k_clamped=h["k_a"] == h["mask_a_stripped"] and h["k_b"] == h["mask_b_stripped"] > 0,
                  first_k_clamped=h["k_a"] == h["mask_a_stripped"] > 1000, one_pixel=h["rows"] == 1, one_whole_block=h["mask_a"] == 512 and h["rows"] == 100)
    assert expect[name], h
    got, header = _run(frame, None if first else model, **kw)
    _assert_rows(got, header, want, False)


@pytest.mark.parametrize("key_bits", [3, 8])
@pytest.mark.parametrize("first", [True, False], ids=["first", "later"])
def test_ties_go_to_the_lower_pixel(first, key_bits):
    """With 3 or 8 key bits every threshold bucket holds ties: exactly k pixels, the lowest indices at the threshold key."""
    frame, model = sc.make_frame()
    kw = dict(sc.SMALL, seed=21, key_bits=key_bits)
    want = sample_oracle(frame, None if first else model, **kw)
    got, header = _run(frame, None if first else model, **kw)
    _assert_rows(got, header, want, False)


def test_ties_in_the_second_round_of_the_block_scan_carry_the_first_rounds_total():
    """512 x 258, every pixel in the mask: 258 blocks, so the last block turns the blocks' tie counts into offsets in two rounds of 256.
    Three key bits put about 64 ties at the threshold key into every block, and k cuts them inside block 256: the ties of blocks 256 and
    257 are chosen or left out by the total the first round carries into the second."""
    H, W, seed, t, cut = 258, 512, 21, 4, 256 * 512 + 300
    pixels = np.arange(H * W)
    frame, _ = sc.blank_frame(H, W, pixels)
    keys = sample_keys(seed, 0, pixels, 3)
    k = int((keys < t).sum() + ((keys == t) & (pixels < cut)).sum())
    kw = dict(sc.DEFAULTS, uniform_sample_num=k, seed=seed, key_bits=3)
    want = sample_oracle(frame, None, **kw)
    assert want["header"]["k_a"] == k == want["header"]["rows"]
    chosen = np.zeros(H * W, bool)
    chosen[want["pixel"]] = True
    assert np.any(chosen[256 * 512:] & (keys[256 * 512:] == t)), "a tie behind the first round's 256 blocks is chosen"
    assert np.any(~chosen[cut:] & (keys[cut:] == t)), "a tie behind the cut is left out"
    got, header = _run(frame, None, **kw)
    _assert_rows(got, header, want, False)


def test_capacity_one_short_sets_overflow_and_writes_nothing_beyond():
    import torch
    import dqo_mapgrowth as mg
    frame, model = sc.make_frame()
    kw = dict(sc.SMALL, seed=11)
    want = sample_oracle(frame, model, **kw)
    cap = want["header"]["rows"] - 1
    buffers = mg.sample_buffers(cap + 8, 16, "cuda")
    for k, v in buffers.items():
        v.fill_(77)
    with pytest.raises(RuntimeError, match="more than"):
        mg.temp_points_init(_cuda(frame), _cuda(model), tick=0, capacity=cap, buffers=buffers, **kw)
    torch.cuda.synchronize()
    header = buffers["header"].tolist()
    assert header[6] == cap and header[7] == 1 and header[:6] == [want["header"][k] for k in mg.SAMPLE_HEADER[:6]]
    short = sample_oracle(frame, model, capacity=cap, **kw)
    for k in EXACT:
        b = buffers[k].cpu().numpy()
        assert np.array_equal(_bits(b[:cap].reshape(short[k].shape)), _bits(short[k])), k
        assert np.all(b[cap:] == 77), k  # the canary behind the capacity
    assert np.all(buffers["rotations"][cap:].cpu().numpy() == 77)


def test_two_calls_on_the_same_buffers_give_the_same_bytes():
    """... whatever the workspace holds: the caller never clears it."""
    import torch
    import _dqo_native as N
    import dqo_mapgrowth as mg
    frame, model = sc.make_frame()
    kw = dict(sc.SMALL, seed=2, tick=0)
    buffers = mg.sample_buffers(mg.sample_capacity(36, 50, False, 300, 2.0, 0.3), 16, "cuda")
    ws = torch.empty((N.lib().dqo_growth_sample_workspace_bytes(50, 36),), dtype=torch.uint8, device="cuda").fill_(0xAB)
    f, m = _cuda(frame), _cuda(model)
    for v in buffers.values():
        v.zero_()
    _, h1 = mg.temp_points_init(f, m, buffers=buffers, workspace=ws, **kw)
    first = {k: v.clone() for k, v in buffers.items()}
    ws.fill_(0x5C)
    _, h2 = mg.temp_points_init(f, m, buffers=buffers, workspace=ws, **kw)
    _, h3 = mg.temp_points_init(f, m, buffers=buffers, workspace=ws, **kw)  # (and on the workspace the call before left)
    torch.cuda.synchronize()
    assert h1 == h2 == h3 and h1["rows"] > 0
    for k, v in buffers.items():
        assert torch.equal(v.view(torch.uint8), first[k].view(torch.uint8)), k


def test_a_full_frame_with_the_reference_defaults_equals_the_oracle():
    """1200 x 680, configs/base.yaml's values (50 000; 0.5 / 0.1 / 0.1; 1.0 / 0.05): 1594 blocks."""
    frame, model = sc.make_frame(680, 1200, seed=3)
    kw = dict(sc.DEFAULTS, seed=2 ** 40 + 17)
    want = sample_oracle(frame, model, **kw)
    assert want["header"]["k_a"] > 10000 and want["header"]["k_b"] > 1000
    got, header = _run(frame, model, **kw)
    _assert_rows(got, header, want, False)


@functools.lru_cache(maxsize=1)
def _mapper_problem():
    import torch
    from test_gpu_mapgrowth import _growth_problem
    dev, cam, scene, settings, gt_color, gt_depth, mask = _growth_problem(20000)
    H, W = gt_depth.shape[-2:]
    rng = np.random.default_rng(8)
    lo, hi = np.asarray(scene["xyz"]).min(0), np.asarray(scene["xyz"]).max(0)
    depth = gt_depth.permute(1, 2, 0).clone()
    depth[:H // 3] += 0.3 * (depth[:H // 3] > 0)       # a depth error in the top third
    depth[H // 2:][depth[H // 2:] == 0] = 2.0           # measurements where the map shows nothing
    normal = rng.normal(size=(H, W, 3)).astype(np.float32)
    inst = np.zeros((H, W, 3), np.float32)
    inst[..., 0] = ((np.arange(W) * 8 // W + 0.5) / 255.0).astype(np.float32)[None, :]  # eight column bands: objects 0..7
    frame = dict(depth_map=depth.contiguous(), color_map=gt_color.permute(1, 2, 0).contiguous(),
                 vertex_map_w=torch.from_numpy(rng.uniform(lo, hi, (H, W, 3)).astype(np.float32)).to(dev),
                 normal_map_w=torch.from_numpy(normal).to(dev), instance_img=torch.from_numpy(inst).to(dev))
    return dev, scene, settings, frame


SAMPLE_KW = dict(uniform_sample_num=3000, error_sample_ratio=0.01)


def test_sample_new_equals_the_oracle_on_its_own_render_and_feeds_grow():
    import torch
    from dqo_harness.fused_mapping import FusedMapper
    dev, scene, settings, frame = _mapper_problem()
    fm = FusedMapper(scene, settings, dev).reserve(6000).track_lifecycle()
    new = fm.sample_new(frame, seed=9, tick=4, **SAMPLE_KW)
    torch.cuda.synchronize()
    out = fm._maintain_ctx.out
    model = dict(render_color=out[0].permute(1, 2, 0), render_depth=out[1].permute(1, 2, 0), render_depth_index=out[3].permute(1, 2, 0),
                 render_transmission=out[6].permute(1, 2, 0))
    want = sample_oracle({k: v.cpu().numpy() for k, v in frame.items()}, {k: v.cpu().numpy() for k, v in model.items()}, seed=9,
                         **dict(sc.DEFAULTS, add_depth_thres=fm.add_depth_thres, **SAMPLE_KW))
    assert want["header"]["k_a"] > 100 and want["header"]["k_b"] > 100
    _assert_rows({k: v.cpu().numpy() for k, v in new.items()}, dict(fm.sample_header), want, False)
    fm.begin_mapping_call()
    stats = fm.grow(new, new_mapping_call=True, tick=4)
    assert stats["candidates"] == want["header"]["rows"] and stats["added"] > 0
    assert int((fm.add_tick == 4).sum().item()) == stats["added"]  # (the map's own rows carry tick 0)


def test_a_shard_keeps_the_unsharded_rows_of_its_objects_in_order():
    import torch
    from dqo_harness.fused_mapping import FusedMapper
    dev, scene, settings, frame = _mapper_problem()
    go = np.asarray(scene["obj_id"], np.int32)
    H, W = int(settings.image_height), int(settings.image_width)
    po = np.broadcast_to((np.arange(W) * 8 // W).astype(np.int32)[None, :], (H, W)).copy()
    whole = FusedMapper(scene, settings, dev).set_object_gate(go, po)
    rows = whole.sample_new(frame, seed=9, tick=4, **SAMPLE_KW)
    out = whole._maintain_ctx.out
    model = dict(render_color=out[0].permute(1, 2, 0), render_depth=out[1].permute(1, 2, 0), render_depth_index=out[3].permute(1, 2, 0),
                 render_transmission=out[6].permute(1, 2, 0))
    assert set(np.unique(go)) == set(range(8)) and rows["xyz"].shape[0] == whole.sample_header["rows"]
    mine = np.isin(go, [2, 5])
    sub = {k: (v[mine] if hasattr(v, "shape") and v.shape[:1] == go.shape else v) for k, v in scene.items()}
    shard = FusedMapper(sub, settings, dev).set_object_gate(go[mine], po)
    kept = shard.sample_new(frame, seed=9, tick=4, model_map=model, **SAMPLE_KW)
    torch.cuda.synchronize()
    sel = (rows["obj_id"] == 2) | (rows["obj_id"] == 5)
    assert 0 < int(sel.sum().item()) < rows["xyz"].shape[0] and shard.sample_header == whole.sample_header
    for k in rows:
        assert torch.equal(kept[k], rows[k][sel]), k
