"""GPU: FusedMapper's per-Gaussian buffers across reserve() and grow() — what a re-allocating step carries for the kept rows and gives
the new ones, that every buffer follows the row count, and what a spare row and a freed row hold.  Small maps; values bit for bit."""
import numpy as np
import pytest

from test_gpu_mapgrowth import _growth_problem

pytestmark = pytest.mark.gpu

PARAMS = ("xyz", "shs", "opacity_raw", "scaling_raw", "rotation_raw")
STATE_KEYS = ("xyz", "shs", "opacity", "scaling", "rotation")
SNAPSHOT = ("init_xyz", "init_scaling", "init_rotation", "attach_mask")
OPTIONAL = ("moment_live", "alive", "gaussian_object", "init_shs", "init_confidence")


def _row_buffers(fm):
    """name -> tensor for every buffer of the mapper that has one row per Gaussian (the ones that exist now)."""
    from dqo_harness.fused_mapping import _ROW_BUFFERS
    assert {b.name for b in _ROW_BUFFERS} >= set(PARAMS + SNAPSHOT + OPTIONAL + ("row_flags", "confidence"))
    out = {(f"{'mv'[b.of[1]]}_{b.of[0]}" if b.of else b.name): a for b, a in fm._rows("param", "moment", "snapshot", "meta", "dropped")}
    assert set(out) >= set(PARAMS + SNAPSHOT + ("row_flags", "confidence") + tuple(f"{s}_{k}" for k in STATE_KEYS for s in "mv"))
    return out


def _assert_row_counts(fm):
    import torch
    from dqo_harness.fused_mapping import _ROW_BUFFERS
    P = fm.P
    bufs = _row_buffers(fm)
    assert len(bufs) >= 21
    for name, a in bufs.items():
        assert torch.is_tensor(a) and a.shape[0] == P, (name, tuple(a.shape), P)
    sized = {b.name: tuple(a.shape) for b, a in fm._rows("sized")}
    assert sized == dict(opacity=(P, 1), scales=(P, 3), rotations=(P, 4), attach_partial=(4 * ((P + 255) // 256),))
    assert len(bufs) + len(sized) == len(list(fm._rows())) <= len(_ROW_BUFFERS)
    assert fm.n_alive + fm._n_spare == P


def _gate(scene, settings, dev):
    """(gaussian_object, pixel_object) of the scene: every pixel is owned by the object of the Gaussian that sets its depth."""
    import torch
    from dqo_harness import mapping
    go = np.asarray(scene["obj_id"], np.int32)
    with torch.no_grad():
        hit = mapping.render(settings, mapping.GaussianParams(scene, dev).activated())["depth_index_map"][0].cpu().numpy()
    return go, np.where(hit >= 0, go[np.clip(hit, 0, None)], -1).astype(np.int32)


def _empty_batch():
    z = lambda *s: np.zeros(s, np.float32)
    return dict(xyz=z(0, 3), scales=z(0, 3), rotations=z(0, 4), opacity=z(0, 1), shs=z(0, 16, 3), obj_id=np.zeros(0, np.int32))


@pytest.mark.parametrize("gated", [False, True])
def test_reallocating_grow_carries_the_mapping_calls_state(gated):
    """grow() WITHOUT new_mapping_call: the mapping call goes on over the compacted map.  The kept rows keep parameters, Adam moments,
    moment_live, init_stat, attach set, row flags and confidence bit for bit and in order; the new rows start with zero moments, zero
    flags and confidence, their own values as init_stat and `opacity < 0.9` as attach membership."""
    import torch
    from dqo_harness import scenes
    from dqo_harness.fused_mapping import FusedMapper
    dev, cam, scene, settings, gt_color, gt_depth, mask = _growth_problem()
    fm = FusedMapper(scene, settings, dev)
    if gated:
        fm.set_object_gate(*_gate(scene, settings, dev))
    fm.set_training_rows(trainable=(torch.arange(fm.P, device=dev) % 5) != 0)
    fm.begin_mapping_call(reset_optimizer=True, history=True)
    fm.capture(gt_color, gt_depth, mask)
    for _ in range(3):
        fm.replay()
    torch.cuda.synchronize()
    assert fm.init_shs is not None and fm._g is not None
    old = {k: v.clone() for k, v in _row_buffers(fm).items()}
    for k in ("m_xyz", "v_xyz", "m_shs", "v_opacity", "moment_live", "confidence", "row_flags", "attach_mask"):
        assert bool((old[k] != 0).any()), k  # (what is carried is not all zeros)
    new = scenes.surfel_room(77, 3000, n_objects=8)
    delete = torch.zeros(fm.P, dtype=torch.bool, device=dev)
    delete[::17] = True
    st = fm.grow(new, delete_mask=delete)
    keep = (~delete).nonzero().reshape(-1)
    nk = keep.numel()
    assert st["added"] > 0 and st["deleted"] == int(delete.sum().item()) and fm.P == nk + st["added"] and "in_place" not in st
    assert torch.equal(st["kept_rows"], keep)
    now = _row_buffers(fm)
    carried = PARAMS + SNAPSHOT + ("row_flags", "confidence", "moment_live") + tuple(f"{s}_{k}" for k in STATE_KEYS for s in "mv")
    for k in carried + (("gaussian_object",) if gated else ()):
        assert torch.equal(now[k][:nk], old[k][keep]), k
    for k in ("row_flags", "confidence", "moment_live") + tuple(f"{s}_{k}" for k in STATE_KEYS for s in "mv"):
        assert not bool((now[k][nk:] != 0).any()), k
    assert torch.equal(fm.init_xyz[nk:], fm.xyz[nk:]) and torch.equal(fm.init_scaling[nk:], fm.scaling_raw[nk:])
    assert torch.equal(fm.init_rotation[nk:], fm.rotation_raw[nk:])
    # the added points among the candidates, by their centres (random, so unique)
    cand = torch.tensor(np.ascontiguousarray(new["xyz"], np.float32), device=dev)
    match = (fm.xyz[nk:, None, :] == cand[None, :, :]).all(dim=2)
    assert bool((match.sum(dim=1) == 1).all())
    src = match.to(torch.uint8).argmax(dim=1)
    cand_opacity = torch.tensor(np.ascontiguousarray(new["opacity"], np.float32), device=dev).reshape(-1)
    assert torch.equal(fm.attach_mask[nk:], (cand_opacity[src] < 0.9).to(torch.uint8))
    if gated:
        assert torch.equal(fm.gaussian_object[nk:], torch.tensor(np.asarray(new["obj_id"], np.int32), device=dev)[src])
    assert fm.attach_count == int(fm.attach_mask.sum().item()) and fm.attach_count > 0
    assert fm.init_shs is None and fm.init_confidence is None
    assert fm._g is None and fm._frames == [] and fm._mixed == {}
    _assert_row_counts(fm)


def test_every_row_buffer_follows_the_row_count():
    import torch
    from dqo_harness import scenes
    from dqo_harness.fused_mapping import FusedMapper
    dev, cam, scene, settings, gt_color, gt_depth, mask = _growth_problem(8000)
    new = scenes.surfel_room(86, 3000, n_objects=8)
    few = {k: np.asarray(v)[:300] for k, v in new.items()}

    def deletions(fm):
        d = torch.zeros(fm.P, dtype=torch.bool, device=dev)
        d[3:8000:19] = True
        return d

    fm = FusedMapper(scene, settings, dev)
    _assert_row_counts(fm)
    fm.begin_mapping_call(history=True)
    _assert_row_counts(fm)
    fm.reserve(2000)
    assert fm.P == 10000 and fm.n_alive == 8000 and fm.init_shs is None
    _assert_row_counts(fm)
    st = fm.grow(few, delete_mask=deletions(fm), new_mapping_call=True)   # in place
    assert st["in_place"] is True and st["added"] > 0 and st["deleted"] > 0 and fm.P == 10000
    assert fm.n_alive == 8000 + st["added"] - st["deleted"]
    _assert_row_counts(fm)
    st = fm.grow(few, new_mapping_call=False)                             # the mapping call goes on: compaction, the same spare rows again
    assert st["in_place"] is False and fm.P == fm.n_alive + 2000
    _assert_row_counts(fm)
    for nmc in (False, True):                                             # a mapper without spare rows
        fm = FusedMapper(scene, settings, dev)
        st = fm.grow(new, delete_mask=deletions(fm), new_mapping_call=nmc)
        assert "in_place" not in st and fm.alive is None and fm.P == 8000 + st["added"] - st["deleted"]
        _assert_row_counts(fm)
    fm = FusedMapper(scene, settings, dev).reserve(16)                    # out of spare rows: compaction and the same number again
    st = fm.grow(new, delete_mask=deletions(fm), new_mapping_call=True)
    assert st["in_place"] is False and st["added"] > 16 and fm.P == fm.n_alive + 16
    assert fm.n_alive == 8000 + st["added"] - st["deleted"]
    _assert_row_counts(fm)
    fm = FusedMapper(scene, settings, dev).set_object_gate(*_gate(scene, settings, dev)).reserve(500)
    assert fm.gaussian_object.shape[0] == 8500
    _assert_row_counts(fm)
    st = fm.grow(few, delete_mask=deletions(fm), new_mapping_call=True)
    assert st["in_place"] is True
    _assert_row_counts(fm)


def test_spare_rows_and_freed_rows_hold_what_the_step_writes():
    """A spare row (reserve) is a parked, tiny, transparent, hidden and frozen Gaussian with zero state.  A row freed by an in-place step
    gets `alive`, the position, opacity, scale, row flags and confidence of a spare row and nothing else: its colour, rotation and
    object id keep their bits (the next Gaussian that takes the row overwrites them)."""
    import torch
    import _dqo_native as N
    from dqo_harness.fused_mapping import FusedMapper
    dev, cam, scene, settings, gt_color, gt_depth, mask = _growth_problem(8000)
    fm = FusedMapper(scene, settings, dev).set_object_gate(*_gate(scene, settings, dev))
    before = {k: v.clone() for k, v in _row_buffers(fm).items()}
    fm.reserve(1000)
    P0, park = 8000, fm._park_position()
    unit_q = torch.tensor([1.0, 0.0, 0.0, 0.0], device=dev)
    spare_value = dict(xyz=park, init_xyz=park, rotation_raw=unit_q, init_rotation=unit_q, opacity_raw=-10.0, scaling_raw=-10.0,
                       init_scaling=-10.0, row_flags=N.ROW_HIDDEN | N.ROW_FROZEN)  # every other buffer: 0
    bufs = _row_buffers(fm)
    assert "alive" in bufs and "gaussian_object" in bufs and "moment_live" in bufs
    for k, a in bufs.items():
        want = spare_value.get(k, 0)
        want = want.to(a.dtype).expand_as(a[P0:]) if torch.is_tensor(want) else torch.full_like(a[P0:], want)
        assert torch.equal(a[P0:], want), k
        if k != "alive":
            assert torch.equal(a[:P0], before[k]), k
    assert bool((fm.alive[:P0] == 1).all()) and fm._n_spare == 1000
    # an in-place step that only deletes: the freed rows stay free
    fm.capture(gt_color, gt_depth, mask)
    for _ in range(3):
        fm.replay()
    torch.cuda.synchronize()
    old = {k: v.clone() for k, v in _row_buffers(fm).items()}
    assert bool((old["confidence"] != 0).any()) and bool((old["m_shs"] != 0).any())
    delete = torch.zeros(fm.P, dtype=torch.bool, device=dev)
    delete[7:P0:13] = True
    graph = fm._g
    st = fm.grow(_empty_batch(), delete_mask=delete, new_mapping_call=True)
    freed = delete.nonzero().reshape(-1)
    assert st["in_place"] is True and st["deleted"] == freed.numel() and st["added"] == 0 and fm._g is graph and not graph.stale
    assert fm._n_spare == 1000 + freed.numel() and fm.n_alive == P0 - freed.numel()
    now = _row_buffers(fm)
    for k in ("alive", "xyz", "opacity_raw", "scaling_raw", "row_flags", "confidence"):
        want = spare_value.get(k, 0)
        want = want.to(now[k].dtype).expand_as(now[k][freed]) if torch.is_tensor(want) else torch.full_like(now[k][freed], want)
        assert torch.equal(now[k][freed], want), k
    for k in ("shs", "rotation_raw", "gaussian_object"):  # not rewritten
        assert torch.equal(now[k][freed], old[k][freed]), k
    rest = (~delete).nonzero().reshape(-1)
    for k in PARAMS + ("alive", "row_flags", "confidence", "gaussian_object"):  # the other rows: untouched
        assert torch.equal(now[k][rest], old[k][rest]), k
    # the new mapping call the step opens: init_stat of the rows as they are now, no moments, freed rows in no attach set
    assert torch.equal(fm.init_xyz, fm.xyz) and torch.equal(fm.init_scaling, fm.scaling_raw) and torch.equal(fm.init_rotation, fm.rotation_raw)
    for k in STATE_KEYS:
        assert not bool((now[f"m_{k}"] != 0).any()) and not bool((now[f"v_{k}"] != 0).any()), k
    assert not bool((fm.moment_live != 0).any()) and not bool((fm.attach_mask[freed] != 0).any())
    assert fm.attach_count == int(fm.attach_mask.sum().item())
    _assert_row_counts(fm)
