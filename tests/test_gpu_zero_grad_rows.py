"""Exact sparse Adam, the list rule of the fused tail: an in-view Gaussian for which the backward marked no partial
gradient record valid — hidden behind an opaque wall of its own object, or gated / masked out while inside the frustum — has a zero
gradient row; with zero moments and outside the attach set it is not updated and keeps moment_live == 0.  Everything the sparse mapper
leaves must be bit for bit what the dense mapper leaves, and the three-kernel form must list the same rows as the fused tail."""
import numpy as np
import pytest

from dqo_harness import scenes

pytestmark = pytest.mark.gpu

W, H, F = 256, 192, 200.0


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available()
    import _dqo_native
    _dqo_native.lib()
    return torch


def _camera(yaw=0.0, pos=(0.0, 0.0, 0.0)):
    return scenes.replica_camera(W, H, F, F, (W - 1) / 2, (H - 1) / 2, yaw=yaw, pitch=0.0, pos=pos)


def _grid(x0, x1, y0, y1, z, step):
    xs, ys = np.arange(x0, x1 + 1e-6, step), np.arange(y0, y1 + 1e-6, step)
    g = np.stack(np.meshgrid(xs, ys, indexing="ij"), -1).reshape(-1, 2)
    return np.concatenate([g, np.full((g.shape[0], 1), z)], 1)


def _scene(hidden_opacity=0.95):
    """Surfels facing the camera at the origin (looking along +z).  Groups (row ranges in the returned dict `rows`):
      wall    three dense opaque layers at z = 2 .. 2.04 over the middle of the image: every pixel they cover exits early inside them
      hidden  a patch at z = 3 behind the middle of the wall, the wall's object: in the frustum, in tile lists, never blended
      side    a patch at z = 2 right of the wall, in plain sight
      front   a patch of ANOTHER object (id 1) at z = 1.2 left of the wall, in plain sight unless the gate gives its pixels to object 0
      behind  Gaussians behind the camera: out of view"""
    rng = np.random.default_rng(5)
    parts = dict(wall=np.concatenate([_grid(-0.8, 0.8, -0.7, 0.7, 2.0 + 0.02 * k, 0.02) for k in range(3)]),
                 hidden=_grid(-0.3, 0.3, -0.25, 0.25, 3.0, 0.05), side=_grid(1.0, 1.2, -0.5, 0.5, 2.0, 0.04),
                 front=_grid(-0.7, -0.6, -0.3, 0.3, 1.2, 0.03), behind=_grid(-1.0, 1.0, -1.0, 1.0, -2.0, 0.1))
    rows, n = {}, 0
    for k, v in parts.items():
        rows[k] = np.arange(n, n + v.shape[0])
        n += v.shape[0]
    xyz = np.concatenate(list(parts.values())).astype(np.float32)
    f = np.float32
    scales = np.tile(np.array([0.03, 0.03, 0.001], f), (n, 1))
    rot = np.tile(np.array([1, 0, 0, 0], f), (n, 1))
    opacity = np.full((n, 1), 0.95, f)
    opacity[rows["wall"]] = 0.99
    opacity[rows["hidden"]] = hidden_opacity
    shs = np.zeros((n, 16, 3), f)
    shs[:, 0, :] = scenes.rgb_to_sh(rng.uniform(0.2, 0.8, (n, 3))).astype(f)
    obj = np.zeros(n, np.int32)
    obj[rows["front"]] = 1
    return dict(xyz=xyz, scales=scales, rotations=rot, opacity=opacity, shs=shs, obj_id=obj), rows


def _target(torch, scene, cam, dev, seed):
    from dqo_harness import mapping
    st = mapping.make_settings(cam, dev)
    rng = np.random.default_rng(seed)
    pert = dict(scene)
    pert["xyz"] = (scene["xyz"] + rng.normal(0, 0.004, scene["xyz"].shape)).astype(np.float32)
    pert["shs"] = scene["shs"].copy()
    pert["shs"][:, 0, :] += rng.normal(0, 0.15, (scene["xyz"].shape[0], 3)).astype(np.float32)
    with torch.no_grad():
        tgt = mapping.render(st, mapping.GaussianParams(pert, dev).activated())
    mask = (tgt["depth_index_map"][0] >= 0).to(torch.uint8).contiguous()
    return st, tgt["render"].clone(), tgt["depth"].clone(), mask


def _equal(torch, a, b, tag):
    for k, pa in a._params().items():
        assert torch.equal(pa, b._params()[k]), (tag, k)
        assert torch.equal(a.state[k][0], b.state[k][0]) and torch.equal(a.state[k][1], b.state[k][1]), (tag, k)
    assert torch.equal(a.opacity, b.opacity) and torch.equal(a.scales, b.scales) and torch.equal(a.rotations, b.rotations), tag
    assert torch.equal(a.confidence, b.confidence), tag


def _moments_zero(torch, fm, rows):
    r = torch.as_tensor(rows, device=fm.device)
    return all(not bool(m[r].any()) and not bool(v[r].any()) for m, v in fm.state.values())


def _mappers(torch, scene, st, dev, gate=None, trainable=None, attach=True):
    """(sparse fused tail, dense fused tail, sparse three-kernel form)"""
    from dqo_harness.fused_mapping import FusedMapper
    ms = [FusedMapper(scene, st, dev, sparse_moments=sp, attach=attach) for sp in (True, False, True)]
    for m in ms:
        if gate is not None:
            m.set_object_gate(*gate)
        if trainable is not None:
            m.set_training_rows(trainable=trainable)
            m.begin_mapping_call()
    return ms


def _run(torch, ms, st, gtc, gtd, mask, n, tag, tile_mask=None, live_log=None):
    """capture at the view `st` (one eager iteration) + n - 1 replays on every mapper; bit-equality after every iteration"""
    sp, de, k3 = ms
    for it in range(n):
        for m, ft in ((sp, True), (de, True), (k3, False)):
            if it == 0:
                m.capture(gtc, gtd, mask, tile_mask=tile_mask, settings=st, fused_tail=ft)
            else:
                m.replay()
        torch.cuda.synchronize()
        assert not sp.graph_overflowed() and not de.graph_overflowed() and not k3.graph_overflowed()
        _equal(torch, sp, de, (tag, it, "sparse vs dense"))
        _equal(torch, sp, k3, (tag, it, "fused tail vs three kernels"))
        assert torch.equal(sp.moment_live, k3.moment_live), (tag, it)
        if live_log is not None:
            live_log.append(sp.moment_live.cpu().numpy().copy())
    assert sp._g.fused_tail and not k3._g.fused_tail


def test_rows_behind_an_opaque_wall_are_not_updated(env):
    torch = env
    dev = torch.device("cuda")
    scene, rows = _scene()
    st, gtc, gtd, mask = _target(torch, scene, _camera(), dev, 11)
    ms = _mappers(torch, scene, st, dev)
    sp = ms[0]
    assert not bool(sp.attach_mask[torch.as_tensor(rows["hidden"], device=dev)].any())
    log = []
    _run(torch, ms, st, gtc, gtd, mask, 3, "front view", live_log=log)
    radii = sp._g.out[8].cpu().numpy()
    assert (radii[rows["hidden"]] > 0).all() and (radii[rows["behind"]] == 0).all()  # hidden: inside the frustum, with tile lists
    live = log[-1]
    assert not live[rows["hidden"]].any() and not live[rows["behind"]].any()
    assert _moments_zero(torch, sp, rows["hidden"])
    assert live[rows["side"]].all() and live[rows["front"]].all() and live[rows["wall"]].mean() > 0.3
    # a view from the side looks past the wall's edge: hidden rows get their first gradient at this iteration and are updated from it on
    # exactly as the dense mapper updates them (bit-equality inside _run)
    cam2 = _camera(yaw=45.0, pos=(2.4, 0.0, 0.6))
    st2, gtc2, gtd2, mask2 = _target(torch, scene, cam2, dev, 12)
    log2 = []
    _run(torch, ms, st2, gtc2, gtd2, mask2, 3, "side view", live_log=log2)
    woke = log2[0][rows["hidden"]] != 0
    assert woke.any(), "the side view must uncover some of the hidden rows"
    assert (log2[-1][rows["hidden"]] >= log2[0][rows["hidden"]]).all()  # a live byte stays
    assert not _moments_zero(torch, sp, rows["hidden"][woke])


def test_rows_hidden_by_the_gate_or_the_tile_mask_are_not_updated(env):
    torch = env
    dev = torch.device("cuda")
    scene, rows = _scene()
    st, gtc, gtd, mask = _target(torch, scene, _camera(), dev, 21)
    # every pixel belongs to object 0: object 1's patch (`front`) is inside the frustum and in plain sight, but acts on no pixel
    pix0 = torch.zeros((H, W), dtype=torch.int32, device=dev)
    gate = (torch.tensor(scene["obj_id"], device=dev), pix0)
    ms = _mappers(torch, scene, st, dev, gate=gate)
    sp = ms[0]
    # ... and a tile mask that drops the right quarter of the image, where `side` lies
    gy, gx = (H + 15) // 16, (W + 15) // 16
    tm = torch.ones((gy, gx), dtype=torch.int32, device=dev)
    tm[:, gx - gx // 4:] = 0
    log = []
    _run(torch, ms, st, gtc, gtd, mask, 3, "gated + masked", tile_mask=tm, live_log=log)
    radii = sp._g.out[8].cpu().numpy()
    assert (radii[rows["front"]] > 0).all()
    live = log[-1]
    assert not live[rows["front"]].any() and not live[rows["hidden"]].any() and _moments_zero(torch, sp, rows["front"])
    masked_side = rows["side"][live[rows["side"]] == 0]
    assert masked_side.size > 0 and _moments_zero(torch, sp, masked_side)
    # the mask goes: `side` gets its first gradients now
    log2 = []
    _run(torch, ms, st, gtc, gtd, mask, 2, "gated", live_log=log2)
    assert log2[0][rows["side"]].all() and not log2[-1][rows["front"]].any()


def test_frozen_rows_and_hidden_attach_members(env):
    torch = env
    dev = torch.device("cuda")
    scene, rows = _scene(hidden_opacity=0.5)  # the hidden patch is in the attach set (opacity < 0.9 at the start of the call)
    st, gtc, gtd, mask = _target(torch, scene, _camera(), dev, 31)
    trainable = torch.ones((scene["xyz"].shape[0],), dtype=torch.bool, device=dev)
    frozen = np.concatenate([rows["hidden"][::2], rows["side"][::3], rows["wall"][::5]])
    trainable[torch.as_tensor(frozen, device=dev)] = False
    ms = _mappers(torch, scene, st, dev, trainable=trainable)
    sp = ms[0]
    before = {k: v.clone() for k, v in sp._params().items()}
    att_hidden = rows["hidden"][1::2]
    assert bool(sp.attach_mask[torch.as_tensor(att_hidden, device=dev)].all())
    log = []
    _run(torch, ms, st, gtc, gtd, mask, 4, "frozen + attach", live_log=log)
    live = log[-1]
    assert live[att_hidden].all()          # in-view attach members are updated, gradient or not
    assert not live[frozen].any() and _moments_zero(torch, sp, frozen)
    fr = torch.as_tensor(frozen, device=dev)
    for k, v in sp._params().items():
        assert torch.equal(v[fr], before[k][fr]), k
    assert not live[rows["behind"]].any()
