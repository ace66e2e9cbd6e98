"""GPU: the whole-map operators' scratch across a change of P (dqo_harness/map_operators.py: _init_operator_state and its per-P half).
Mapper A has run every operator before the map is re-allocated, mapper B has not: afterwards A works on scratch that survived the resize
(or was dropped by it), B on first-use scratch, and everything they return must agree byte for byte.  A buffer that is sized by P and
survives the resize, or a context that is not sized anew, shows here.  The image is the lifecycle tests' 1200 x 680, both sides above 160,
so MS-SSIM is included."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TH = dict(stable_confidence_thres=2.0, unstable_time_window=100, add_color_thres=0.1, add_depth_thres=0.1, delete_thresh=1)


def _mapper(scene, settings, dev, H, W):
    import torch
    from dqo_harness.fused_mapping import FusedMapper
    fm = FusedMapper(scene, settings, dev)
    fm.set_object_gate(np.asarray(scene["obj_id"], np.int32), np.zeros((H, W), np.int32))
    fm.track_lifecycle(stable_mask=torch.arange(fm.P, device=dev) % 2 == 0, tick=0, frame_id=3)
    fm.frame_id.copy_((3 + torch.arange(fm.P, device=dev) % 4).to(torch.int32))  # ids 3..6: the window (4, 6] holds half of the rows
    assert fm.alive is None and fm._n_spare == 0
    return fm


def test_scratch_that_survived_a_resize_equals_first_use_scratch():
    import torch
    import dqo_eval
    from dqo_harness import scenes
    from test_gpu_lifecycle import _problem
    dev, cam, scene, settings, gt_color, gt_depth, mask = _problem()
    H, W = gt_depth.shape[-2], gt_depth.shape[-1]
    a, b = _mapper(scene, settings, dev, H, W), _mapper(scene, settings, dev, H, W)
    # a frame that disagrees with the map (test_gpu_lifecycle's): the top third lies 0.5 further away, the bottom third is 0.3 brighter
    gt_d = gt_depth.clone()
    gt_d[:, :H // 3] += 0.5 * (gt_d[:, :H // 3] > 0)
    gt_c = gt_color.clone()
    gt_c[:, 2 * H // 3:] += 0.3
    frames = [(None, gt_color, gt_depth), (settings, gt_c, gt_d)]
    rng = np.random.default_rng(3)
    gt_points = torch.tensor((np.asarray(scene["xyz"], np.float32)[::2] + rng.normal(0, 0.02, (4000, 3))).astype(np.float32), device=dev)
    gt_object = torch.tensor(np.asarray(scene["obj_id"], np.int32)[::2], device=dev)
    projection = torch.tensor(cam.projection_matrix, dtype=torch.float32, device=dev)

    def read_only(fm):
        """The operators that leave the map as it is, once each: what each returns, cloned."""
        ms = torch.zeros((2, 20), dtype=torch.float32, device=dev)
        got = dict(evaluate=fm.evaluate(frames).clone(), evaluate_ms=fm.evaluate_ms_ssim(frames, ms).clone(), ms_ssim=ms)
        table, header = fm.pack_rows()
        torch.cuda.synchronize()
        n = int(header.sum().item())
        assert n == fm.n_alive
        got.update(pack_header=header.clone(), pack_table=table[:n].clone())  # (rows at and behind U + S keep their bytes)
        got["objects"] = fm.evaluate_geometry_objects(gt_points, gt_object, (0.02, 0.05)).clone()
        return got

    first = read_only(a)
    a.make_mesh([None, settings], dqo_eval.TsdfVolume((-1.0, -1.0, 0.2), 0.25, (16, 16, 16), 0.5, dev))
    stats = a.prune_floaters(gt_depth, (5, 5), projection=projection).clone()  # (an empty window: nothing is deleted)
    torch.cuda.synchronize()
    assert stats[1:3].tolist() == [0, 0] and a.n_alive == a.P == 8000
    untouched = {n.name: y for n, y in b._rows("param", "meta")}
    for n, x in a._rows("param", "meta"):
        if n.name != "alive":  # (prune_floaters made it: all ones)
            assert torch.equal(x, untouched[n.name]), n.name

    new = {k: np.asarray(v)[:300] for k, v in scenes.surfel_room(86, 3000, n_objects=8).items()}
    for fm in (a, b):
        st = fm.grow(new, new_mapping_call=True, tick=9)
        assert st["added"] > 0 and st.get("in_place") is not True and fm.P == 8000 + st["added"]
        fm.add_tick[1::50] = -200  # (unstable rows that have been around for too long)
    assert a.P == b.P and a._maintain_ctx is None and a._prune_ctx is None and a._checkpoint == {}

    got = []
    for fm in (a, b):
        r = read_only(fm)
        r["maintain"] = fm.maintain(10, gt_c, gt_d, **TH).clone()
        r["prune"] = fm.prune_floaters(gt_depth, (4, 6), projection=projection).clone()
        torch.cuda.synchronize()
        assert not fm.maintain_overflowed() and not fm.prune_overflowed()
        got.append(r)
    ra, rb = got
    assert sum(ra["maintain"][2:5].tolist()) > 0 and ra["prune"][0].item() > 0 and sum(ra["prune"][1:3].tolist()) > 0  # both deleted rows
    assert not torch.equal(ra["evaluate"], first["evaluate"])  # (the map did change in between)
    for k in ra:
        assert ra[k].dtype == rb[k].dtype and ra[k].shape == rb[k].shape, k
        assert ra[k].cpu().numpy().tobytes() == rb[k].cpu().numpy().tobytes(), k
    rows_a, rows_b = list(a._rows()), list(b._rows())
    assert [n.name for n, _ in rows_a] == [n.name for n, _ in rows_b]
    for (n, x), (_, y) in zip(rows_a, rows_b):
        assert x.shape == y.shape and x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes(), n.name
