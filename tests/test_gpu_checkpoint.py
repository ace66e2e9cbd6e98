"""Map checkpoints on the GPU (csrc/map_checkpoint.hip; dqo_ply.pack_rows / unpack_rows; FusedMapper.pack_rows / save_model / load_model /
from_model_ply).  The expectation is never computed by the code under test: the buffers are indexed in torch on the device by
alive & ~stable and by alive & stable, copied to numpy and handed to the existing dqo_ply.save_model_ply.  FILE BYTES and the header counts
are compared exactly, tables as uint32 views; the buffers hold random bit patterns (NaNs with payloads, infinities, -0, denormals), so a
value-dependent path shows."""
import os

import numpy as np
import pytest

from checkpoint_cases import values

pytestmark = pytest.mark.gpu

SENTINEL = 0x5EA7AB1E


def _device_map(P, M, seed):
    import torch
    dev = torch.device("cuda")
    return {k: torch.from_numpy(a).to(dev) for k, a in values(P, M, seed).items()}


def _expected_files(prefix, v, alive, stable, with_conf, conf_null=False):
    """path.ply / path_stable.ply of the two clouds through dqo_ply.save_model_ply; returns (U, S)."""
    import torch
    import dqo_ply
    P = v["xyz"].shape[0]
    live = torch.ones((P,), dtype=torch.bool, device=v["xyz"].device) if alive is None else alive != 0
    st = torch.zeros_like(live) if stable is None else stable != 0
    counts = []
    for name, sel in ((prefix + ".ply", live & ~st), (prefix + "_stable.ply", live & st)):
        pick = lambda k: v[k][sel].cpu().numpy()
        dqo_ply.save_model_ply(name, pick("xyz"), pick("shs"), pick("opacity_raw"), pick("scaling_raw"), pick("rotation_raw"),
                               None if conf_null else pick("confidence"), include_confidence=with_conf)
        counts.append(int(sel.sum().item()))
    return tuple(counts)


def _read(path):
    return open(path, "rb").read() if os.path.exists(path) else None


def _vertex_bytes(blob):
    return b"" if blob is None else blob[blob.index(b"end_header\n") + len(b"end_header\n"):]


def _masks(P, rng):
    """name -> (alive, stable) as uint8 arrays or None.  Flags are 'non-zero', not 'one'."""
    rnd = lambda p: (rng.random(P) < p).astype(np.uint8) * rng.choice(np.array([1, 2, 200], np.uint8), size=P)
    block = np.arange(P) // 256
    last = block == block[-1]
    cases = {
        "both NULL": (None, None),
        "alive NULL": (None, rnd(0.4)),
        "stable NULL": (rnd(0.7), None),
        "random": (rnd(0.7), rnd(0.4)),
        "all stable": (rnd(0.8), np.full(P, 3, np.uint8)),
        "nothing alive": (np.zeros(P, np.uint8), rnd(0.5)),
        "a block without a live row": ((rnd(0.7) * (block != 1)).astype(np.uint8), rnd(0.5)),
        "a block of one cloud next to a block of the other": (np.ones(P, np.uint8), (block % 2).astype(np.uint8)),
        "live rows only in the last partial block": ((rnd(0.6) * last).astype(np.uint8), rnd(0.5)),
    }
    return cases


def _pack_case(tmp_path, v, alive, stable, with_conf, conf_null, tag):
    import torch
    import dqo_ply
    dev = v["xyz"].device
    P, M = v["shs"].shape[:2]
    C = 6 + 3 * M + 8 + (1 if with_conf else 0)
    ws = dqo_ply.pack_workspace(P, dev)
    runs = []
    for _ in range(2):  # the same workspace twice, no zero fill in between
        table = torch.full((P + 3, C), SENTINEL, dtype=torch.int32, device=dev).view(torch.float32)
        header = torch.full((2,), -7, dtype=torch.int32, device=dev)
        out = dqo_ply.pack_rows(v["xyz"], v["shs"], v["opacity_raw"], v["scaling_raw"], v["rotation_raw"], None if conf_null else v["confidence"],
                                alive, stable, with_conf, out=table, header=header, workspace_buffer=ws)
        assert out[0] is table and out[1] is header
        torch.cuda.synchronize()
        assert not ws[:4352].any(), (tag, "the ticket words came back at zero")
        runs.append((table.view(torch.int32).cpu().numpy().view(np.uint32), header.cpu().numpy()))
    (t0, h0), (t1, h1) = runs
    assert t0.tobytes() == t1.tobytes() and h0.tobytes() == h1.tobytes(), tag
    want = str(tmp_path / "want")
    U, S = _expected_files(want, v, alive, stable, with_conf, conf_null)
    assert (int(h0[0]), int(h0[1])) == (U, S), tag
    assert (t0[U + S:] == SENTINEL).all(), (tag, "rows behind U + S keep their bytes")
    got = str(tmp_path / "got")
    rows = t0.view(np.float32)
    assert dqo_ply.write_vertex_table(got + ".ply", rows[:U], 3 * (M - 1), with_conf) == U
    assert dqo_ply.write_vertex_table(got + "_stable.ply", rows[U:U + S], 3 * (M - 1), with_conf) == S
    for name in (".ply", "_stable.ply"):
        w, g = _read(want + name), _read(got + name)
        assert w == g, (tag, name)
        for f in (want + name, got + name):
            if os.path.exists(f):
                os.remove(f)
        if w is not None:  # ... and as a table of 32-bit words
            lo, n = (0, U) if name == ".ply" else (U, S)
            assert np.array_equal(np.frombuffer(_vertex_bytes(w), np.uint32).reshape(n, C), t0[lo:lo + n]), (tag, name)
    return U, S


# 8192 + 300 rows: 34 count blocks, so dqo_ticket_take uses two ticket lines.  256 * 256 + 5 rows: 257 count blocks, so the last block's
# scan takes a second round of 256 pairs with a carried total (the scan does not depend on the row width: M = 1).
@pytest.mark.parametrize("conf", ["confidence", "no column", "NULL"])
@pytest.mark.parametrize("P, M", [(P, M) for P in (1, 255, 256, 257, 3 * 256 + 17, 8192 + 300) for M in (1, 4, 16)] + [(256 * 256 + 5, 1)])
def test_pack_rows_is_save_model_ply_of_the_indexed_buffers(tmp_path, P, M, conf):
    import torch
    v = _device_map(P, M, 1000 * M + P)
    rng = np.random.default_rng(P + M)
    seen = set()
    for name, (alive, stable) in _masks(P, rng).items():
        t = lambda a: None if a is None else torch.from_numpy(a).to(v["xyz"].device)
        U, S = _pack_case(tmp_path, v, t(alive), t(stable), conf != "no column", conf == "NULL", (P, M, conf, name))
        seen.add((U > 0, S > 0))
        if name == "nothing alive":
            assert (U, S) == (0, 0)
    assert (False, False) in seen and (True, False) in seen and (P < 2 or (True, True) in seen)


@pytest.mark.parametrize("M", [1, 4, 16])
@pytest.mark.parametrize("n, first_row, P", [(1, 0, 1), (63, 5, 70), (64, 0, 64), (65, 200, 300), (3 * 256 + 17, 100, 1000)])
def test_unpack_rows_inverts_pack_rows(n, first_row, P, M):
    import torch
    import dqo_ply
    src = _device_map(n, M, 7 * M + n)
    for with_conf in (True, False):
        table, header = dqo_ply.pack_rows(src["xyz"], src["shs"], src["opacity_raw"], src["scaling_raw"], src["rotation_raw"], src["confidence"],
                                          None, None, with_conf)
        dst = {k: torch.full((P,) + tuple(a.shape[1:]), SENTINEL, dtype=torch.int32, device=a.device).view(torch.float32)
               for k, a in src.items()}
        dqo_ply.unpack_rows(table, first_row, dst["xyz"], dst["shs"], dst["opacity_raw"], dst["scaling_raw"], dst["rotation_raw"],
                            dst["confidence"])
        torch.cuda.synchronize()
        assert header.tolist() == [n, 0]
        for k, a in dst.items():
            got = a.view(torch.int32).cpu().numpy().view(np.uint32)
            want = src[k].view(torch.int32).cpu().numpy().view(np.uint32)
            if k == "confidence" and not with_conf:
                want = np.zeros_like(want)  # a table without the column writes zeros
            assert np.array_equal(got[first_row:first_row + n], want), (k, with_conf)
            assert (got[:first_row] == SENTINEL).all() and (got[first_row + n:] == SENTINEL).all(), (k, with_conf)


# ---- FusedMapper ------------------------------------------------------------------------------------------------------------------------
def _mapper(P=600, spare=300, seed=17, **kw):
    import torch
    from dqo_harness import mapping, scenes
    from dqo_harness.fused_mapping import FusedMapper
    dev = torch.device("cuda")
    cam = scenes.Camera(160, 120, 131.25, 131.25, 79.5, 59.5, scenes.rot_yx(7.0, -3.0), np.array([0.05, -0.02, 0.1]))
    scene = scenes.frustum_cloud(seed, P, cam)
    st = mapping.make_settings(cam, dev)
    fm = FusedMapper(scene, st, dev, **kw)
    fm.reserve(spare)
    return dev, cam, scene, st, fm


def _mapper_buffers(fm):
    return dict(xyz=fm.xyz, shs=fm.shs, opacity_raw=fm.opacity_raw, scaling_raw=fm.scaling_raw, rotation_raw=fm.rotation_raw,
                confidence=fm.confidence.reshape(-1, 1))


def _expected_save(prefix, fm):
    """The six files by the reference's rules (mapper.py:1580-1608), through save_model_ply and a concatenation of its tables."""
    v = _mapper_buffers(fm)
    want = {}
    for with_conf, tag in ((True, ""), (False, "_sibr")):
        base = prefix + "_tmp"
        U, S = _expected_files(base, v, fm.alive, fm.stable, with_conf)
        a, b = _read(base + ".ply"), _read(base + "_stable.ply")
        for f in (base + ".ply", base + "_stable.ply"):
            if os.path.exists(f):
                os.remove(f)
        if a is not None:
            want[prefix + tag + ".ply"] = (U, a)
        if b is not None:
            want[prefix + "_stable" + tag + ".ply"] = (S, b)
        if a is not None and b is not None:
            head = a[:a.index(b"end_header\n") + len(b"end_header\n")].replace(b"element vertex %d\n" % U, b"element vertex %d\n" % (U + S))
            want[prefix + "_merge" + tag + ".ply"] = (U + S, head + _vertex_bytes(a) + _vertex_bytes(b))
    return want


@pytest.mark.parametrize("situation", ["both clouds", "only unstable", "only stable", "lifecycle untracked"])
def test_save_model_writes_the_references_files(tmp_path, situation):
    import torch
    dev, cam, scene, st, fm = _mapper()
    P = fm.P
    g = torch.Generator(device="cpu").manual_seed(3)
    fm._free_rows(torch.tensor([3, 4, 5, 260, 599], device=dev))  # spare rows among the live ones
    fm.confidence.copy_(torch.rand((P,), generator=g).to(dev) * 700 * (fm.alive != 0))
    if situation != "lifecycle untracked":
        mask = {"both clouds": torch.rand((P,), generator=g) < 0.4, "only unstable": torch.zeros((P,), dtype=torch.bool),
                "only stable": torch.ones((P,), dtype=torch.bool)}[situation]
        fm.track_lifecycle(stable_mask=mask.to(dev))
    prefix = str(tmp_path / "iter_0007")
    want = _expected_save(prefix, fm)
    kinds = {"both clouds": 6, "only unstable": 2, "only stable": 2, "lifecycle untracked": 2}
    assert len(want) == kinds[situation]
    fm.pack_rows()  # (the first call allocates)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        table, header = fm.pack_rows(include_confidence=False)  # no synchronisation, nothing read back
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert table.shape == (P, 6 + 3 * fm.M + 8) and table.is_cuda and header.is_cuda
    got = fm.save_model(prefix)
    assert set(os.listdir(tmp_path)) == {os.path.basename(f) for f in want}
    assert got == {f: n for f, (n, _) in want.items()}
    for f, (n, blob) in want.items():
        assert _read(f) == blob, os.path.basename(f)
    if situation == "both clouds":  # the merged files are the two others' vertex data, one after the other
        for tag in ("", "_sibr"):
            assert _vertex_bytes(_read(prefix + "_merge" + tag + ".ply")) == (_vertex_bytes(_read(prefix + tag + ".ply")) +
                                                                               _vertex_bytes(_read(prefix + "_stable" + tag + ".ply")))
    # the switches
    for f in got:
        os.remove(f)
    only = fm.save_model(prefix, save_sibr=False, save_merge=False)
    assert set(only) == {f for f in want if "_sibr" not in f and "_merge" not in f} == {os.path.join(tmp_path, f) for f in os.listdir(tmp_path)}
    assert fm.save_model(prefix, save_data=False, save_sibr=False) == {}


def test_round_trip_through_from_model_ply(tmp_path):
    import torch
    import _dqo_native as N
    from dqo_harness.fused_mapping import FusedMapper
    dev, cam, scene, st, fm = _mapper()
    g = torch.Generator(device="cpu").manual_seed(5)
    fm._free_rows(torch.tensor([0, 7, 300], device=dev))
    fm.confidence.copy_(torch.rand((fm.P,), generator=g).to(dev) * 700 * (fm.alive != 0))
    fm.track_lifecycle(stable_mask=(torch.rand((fm.P,), generator=g) < 0.5).to(dev), tick=3)
    a = str(tmp_path / "a")
    saved = fm.save_model(a)
    U, S = saved[a + ".ply"], saved[a + "_stable.ply"]
    assert U > 0 and S > 0 and U + S == 597
    fm2 = FusedMapper.from_model_ply(a + ".ply", a + "_stable.ply", st, dev, spare_rows=50, tick=11)
    n, P2 = U + S, U + S + 50
    assert fm2.P == P2 and fm2.M == fm.M
    b = str(tmp_path / "b")
    again = fm2.save_model(b)
    assert {os.path.basename(k)[1:]: v for k, v in again.items()} == {os.path.basename(k)[1:]: v for k, v in saved.items()}
    for f in saved:
        assert _read(f) == _read(b + f[len(a):]), f
    # the loaded mapper's state
    live = torch.arange(P2, device=dev) < n
    assert torch.equal(fm2.alive != 0, live)
    assert torch.equal(fm2.stable, ((torch.arange(P2, device=dev) >= U) & live).to(torch.uint8))
    assert torch.equal(fm2.add_tick, live.to(torch.int32) * 11)
    assert not fm2.depth_error_counter.any() and not fm2.color_error_counter.any()
    order = torch.cat([torch.nonzero((fm.alive != 0) & (fm.stable == 0)).reshape(-1), torch.nonzero((fm.alive != 0) & (fm.stable != 0)).reshape(-1)])
    bits = lambda t: t.contiguous().view(torch.int32)
    assert torch.equal(bits(fm2.confidence[:n]), bits(fm.confidence[order])) and not fm2.confidence[n:].any()
    for k in ("xyz", "shs", "opacity_raw", "scaling_raw", "rotation_raw"):  # raw, straight from the file: no clamp, no log
        assert torch.equal(bits(getattr(fm2, k)[:n]), bits(getattr(fm, k)[order])), k
    for pair in fm2.state.values():
        assert not pair[0].any() and not pair[1].any()
    assert not fm2.moment_live.any() and fm2.step_count == 0
    # the spare rows: parked and flagged as _free_rows leaves them
    assert torch.equal(fm2.xyz[n:], fm2._park_position().expand(50, 3))
    assert (fm2.opacity_raw[n:] == -10).all() and (fm2.scaling_raw[n:] == -10).all()
    assert (fm2.row_flags[n:] == (N.ROW_HIDDEN | N.ROW_FROZEN)).all() and not fm2.row_flags[:n].any()
    assert fm2._n_spare == 50
    # a file without the confidence column loads zeros
    fm2.load_model(a + "_sibr.ply", a + "_stable_sibr.ply")
    assert not fm2.confidence.any() and torch.equal(bits(fm2.xyz[:n]), bits(fm.xyz[order])) and not fm2.add_tick.any()
    # one file alone: the other cloud is empty
    fm2.load_model(None, a + "_stable.ply", tick=2)
    assert int((fm2.alive != 0).sum()) == S and torch.equal(fm2.stable != 0, fm2.alive != 0) and fm2._n_spare == P2 - S
    assert torch.equal(bits(fm2.confidence[:S]), bits(fm.confidence[order[U:]]))
    # too many rows
    dev3, _, _, _, small = _mapper(P=100, spare=20)
    with pytest.raises(RuntimeError, match=r"reserve\(%d\)" % (n - 120)):
        small.load_model(a + ".ply", a + "_stable.ply")
    assert small.P == 120


def test_a_saved_map_evaluates_the_same_after_loading(tmp_path):
    """No spare rows and one cloud: the row order is the identity, so the loaded mapper IS the saved one."""
    import torch
    from dqo_harness import mapping, scenes
    from dqo_harness.fused_mapping import FusedMapper
    dev = torch.device("cuda")
    cams = [scenes.Camera(160, 120, 131.25, 131.25, 79.5, 59.5, scenes.rot_yx(yaw, pitch), np.array(t))
            for yaw, pitch, t in ((7.0, -3.0, [0.05, -0.02, 0.1]), (3.0, 1.0, [-0.1, 0.03, 0.2]))]
    scene = scenes.frustum_cloud(17, 4000, cams[0])
    settings = [mapping.make_settings(c, dev) for c in cams]
    targets = [mapping.perturbed_target(scene, s, dev, 40 + k) for k, s in enumerate(settings)]
    frames = [(None if k == 0 else s, t["gt_color"], t["gt_depth"]) for k, (s, t) in enumerate(zip(settings, targets))]
    fm = FusedMapper(scene, settings[0], dev)
    before = fm.evaluate(frames).view(torch.int32).cpu().numpy().copy()
    prefix = str(tmp_path / "map")
    assert fm.save_model(prefix, save_sibr=False) == {prefix + ".ply": 4000}
    other = FusedMapper(scenes.frustum_cloud(99, 4000, cams[0]), settings[0], dev)
    assert other.evaluate(frames).view(torch.int32).cpu().numpy().tobytes() != before.tobytes()
    other.load_model(prefix + ".ply")
    assert other.evaluate(frames).view(torch.int32).cpu().numpy().tobytes() == before.tobytes()
    fresh = FusedMapper.from_model_ply(prefix + ".ply", None, settings[0], dev)
    assert fresh.evaluate(frames).view(torch.int32).cpu().numpy().tobytes() == before.tobytes()
    assert np.isfinite(before.view(np.float32)).all()
