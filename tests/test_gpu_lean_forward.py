"""The training form of the forward (dqo_rast_forward_train; blend_forward_kernel<.., AUX = false>): FusedMapper records iterations
1 .. k-1 of an unrolled graph without the six auxiliary outputs (hit colour id / weight, hit depth id / weight, T, n_touched), which
the next iteration would overwrite unread.  Everything a caller can observe after a launch must be what k single-iteration launches
leave, bit for bit; and the lean iteration must leave the auxiliary outputs alone."""
import numpy as np
import pytest

from dqo_harness import scenes

pytestmark = pytest.mark.gpu

AUX = (2, 3, 4, 5, 6, 7)  # of the op's nine outputs: hit_color, hit_depth, hit_color_weight, hit_depth_weight, T_map, n_touched


@pytest.fixture(scope="module")
def problem():
    """3 000 Gaussians on 64 x 48, three object ids in vertical bands 12 pixels wide (the bands cut 8 x 8 quadrants: mixed ones), one
    tile masked out; 90 % of the opacities are 0.99, above the opaque threshold: depth hits."""
    import torch
    assert torch.cuda.is_available()
    from dqo_harness import mapping
    P = 3000
    cam = scenes.Camera(64, 48, 60.0, 60.0, 31.5, 23.5)
    scene = scenes.frustum_cloud(21, P, cam, zmin=0.6, zmax=4.0)
    dev = torch.device("cuda")
    settings = mapping.make_settings(cam, dev)
    rng = np.random.default_rng(22)
    pert = dict(scene)
    pert["xyz"] = (scene["xyz"] + rng.normal(0, 0.004, scene["xyz"].shape)).astype(np.float32)
    pert["shs"] = scene["shs"].copy()
    pert["shs"][:, 0, :] += rng.normal(0, 0.15, (P, 3)).astype(np.float32)
    with torch.no_grad():
        tgt = mapping.render(settings, mapping.GaussianParams(pert, dev).activated())
    mask = torch.tensor(rng.uniform(size=(cam.H, cam.W)) < 0.8, device=dev) & (tgt["depth_index_map"][0] >= 0)
    assert (tgt["depth_index_map"][0] >= 0).float().mean().item() > 0.5  # depth hits occur
    tile_mask = torch.ones((3, 4), dtype=torch.int32, device=dev)
    tile_mask[1, 2] = 0
    go = (np.arange(P) % 3).astype(np.int32)
    po = np.broadcast_to(((np.arange(cam.W) // 12) % 3).astype(np.int32), (cam.H, cam.W)).copy()
    return dict(torch=torch, scene=scene, settings=settings, dev=dev, gt_color=tgt["render"].clone(), gt_depth=tgt["depth"].clone(), mask=mask,
                tile_mask=tile_mask, gate=(go, po))


def _mapper(pb, gated, unroll):
    from dqo_harness.fused_mapping import FusedMapper
    fm = FusedMapper(pb["scene"], pb["settings"], pb["dev"])
    if gated:
        fm.set_object_gate(*pb["gate"])
    fm.capture(pb["gt_color"], pb["gt_depth"], pb["mask"], tile_mask=pb["tile_mask"], unroll=unroll)
    assert fm._g.tap is not None and fm._g.fused_tail  # (the path whose inner iterations are recorded lean)
    return fm


def _assert_same_state(torch, a, b, outputs=range(9)):
    for i in outputs:
        assert torch.equal(a._g.out[i], b._g.out[i]), f"output {i}"
    assert torch.equal(a.loss, b.loss)
    for k, pa in a._params().items():
        assert torch.equal(pa, b._params()[k]), k
        assert torch.equal(a.state[k][0], b.state[k][0]) and torch.equal(a.state[k][1], b.state[k][1]), k
    assert torch.equal(a.moment_live, b.moment_live) and torch.equal(a.confidence, b.confidence)
    assert a.step_count == b.step_count and int(a._g.step_dev.item()) == int(b._g.step_dev.item())


@pytest.mark.parametrize("gated", [True, False], ids=["gate", "no-gate"])
def test_unrolled_graph_with_lean_inner_iterations_is_bitwise_single_iterations(problem, gated):
    torch = problem["torch"]
    a, b = _mapper(problem, gated, 3), _mapper(problem, gated, 1)
    if gated:  # at least one quadrant with more than one owner, and the masked tile is there
        po = torch.as_tensor(problem["gate"][1])
        assert any(len(torch.unique(po[y:y + 8, x:x + 8])) > 1 for y in range(0, 48, 8) for x in range(0, 64, 8))
    a.replay()
    for _ in range(3):
        b.replay()
    torch.cuda.synchronize()
    assert not a.graph_overflowed() and not b.graph_overflowed()
    assert a.step_count == 4 and (a._g.out[7] != 0).any() and (a._g.out[3] >= 0).any()
    _assert_same_state(torch, a, b)
    if not gated:
        return
    # (c) the last iteration of the unrolled graph writes the auxiliary outputs ...
    for i in AUX:
        a._g.out[i].fill_(-7)
    a.replay()
    for _ in range(3):
        b.replay()
    torch.cuda.synchronize()
    _assert_same_state(torch, a, b)
    # ... and a lean iteration does not touch them: the graph's calls issued eagerly, cut behind the first (lean) iteration
    c = _mapper(problem, gated, 1)
    for i in AUX:
        c._g.out[i].fill_(-7)
    c._static_iteration(lean=True)
    torch.cuda.synchronize()
    assert not c.graph_overflowed()
    for i in AUX:
        assert bool((c._g.out[i] == -7).all()), f"output {i} was written by the lean iteration"
    # (its colour, depth and radii are the full iteration's)
    d = _mapper(problem, gated, 1)
    d._static_iteration()
    torch.cuda.synchronize()
    for i in (0, 1, 8):
        assert torch.equal(c._g.out[i], d._g.out[i]), f"output {i}"
    assert torch.equal(c.loss, d.loss)
    for k, pc in c._params().items():
        assert torch.equal(pc, d._params()[k]), k
