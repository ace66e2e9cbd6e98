"""csrc/map_tsdf.hip on the GPU, bit for bit against tests/tsdf_oracle.py: the integration of three analytic RGB-D frames into a
40 x 36 x 28 volume (no side a multiple of the block size), the extraction of the oracle test's sphere and of the integrated volume
(order included, capacities, guard words, repeatability) and FusedMapper.make_mesh against TsdfVolume.integrate applied by hand."""
import functools
import math

import numpy as np
import pytest

import tsdf_oracle as O

pytestmark = pytest.mark.gpu

DIMS, L, TRUNC = (40, 36, 28), np.float32(0.05), np.float32(0.15)
ORIGIN = (np.float32(-1.0), np.float32(-0.9), np.float32(0.6))
W, H, FX, FY, CX, CY = 64, 48, 40.0, 42.0, 31.5, 23.5
DEPTH_TRUNC = 1.75
PLANE_Z, SPHERE_C, SPHERE_R = 1.7, np.array([0.1, 0.0, 1.3]), 0.3


def _rot(yaw, pitch):
    y, p = math.radians(yaw), math.radians(pitch)
    Ry = np.array([[math.cos(y), 0, math.sin(y)], [0, 1, 0], [-math.sin(y), 0, math.cos(y)]])
    Rx = np.array([[1, 0, 0], [0, math.cos(p), -math.sin(p)], [0, math.sin(p), math.cos(p)]])
    return Rx @ Ry


def _frame(yaw, pitch, pos, k):
    """(depth [H,W], color [3,H,W], w2c [4,4]) float32 of the scene — the plane z = PLANE_Z with a sphere in front — seen from a camera
    at `pos`: the analytic ray cast, in double, rounded once.  A block of pixels has no depth (0)."""
    R = _rot(yaw, pitch)
    w2c = np.eye(4)
    w2c[:3, :3], w2c[:3, 3] = R, -R @ np.asarray(pos, float)
    u, v = np.meshgrid(np.arange(W, dtype=float), np.arange(H, dtype=float))
    dc = np.stack([(u - CX) / FX, (v - CY) / FY, np.ones_like(u)], -1)  # camera rays with z = 1: the ray parameter is the depth
    dw = dc @ R  # R^T dc
    o = np.asarray(pos, float)
    with np.errstate(all="ignore"):
        tp = (PLANE_Z - o[2]) / dw[..., 2]
        tp = np.where(tp > 0, tp, 0.0)
        oc = o - SPHERE_C
        a, b, c = (dw * dw).sum(-1), 2 * (dw @ oc), oc @ oc - SPHERE_R ** 2
        disc = b * b - 4 * a * c
        ts = np.where(disc > 0, (-b - np.sqrt(np.abs(disc))) / (2 * a), 0.0)
        ts = np.where(ts > 0, ts, 0.0)
    depth = np.where((ts > 0) & ((ts < tp) | (tp == 0)), ts, tp)
    depth[5:9, 40:47] = 0.0  # no measurement
    color = np.stack([0.5 + 0.5 * np.sin(0.2 * u + k), 0.5 + 0.5 * np.cos(0.15 * v - k), (u + 2 * v) / (W + 2 * H)])
    return depth.astype(np.float32), color.astype(np.float32), w2c.astype(np.float32)


@functools.lru_cache(maxsize=1)
def scene():
    """Three frames and the oracle's volume after each.  Pose 0 looks along +z from the origin: the grid's near corners lie outside the
    image.  Pose 1 is turned and shifted: part of the plane is deeper than DEPTH_TRUNC.  Pose 2 stands INSIDE the grid: part of the grid
    is behind the camera."""
    frames = [_frame(0.0, 0.0, (0.0, 0.0, 0.0), 0), _frame(14.0, -9.0, (0.35, -0.2, 0.1), 1), _frame(-35.0, 6.0, (-0.7, 0.1, 0.95), 2)]
    vol, states = O.clear(DIMS), []
    px, py, pz = O.centres(ORIGIN, L, DIMS)
    for depth, color, w2c in frames:
        before = vol["weight"].copy()
        O.integrate(vol, ORIGIN, L, TRUNC, depth, color, FX, FY, CX, CY, w2c, DEPTH_TRUNC)
        states.append({k: v.copy() for k, v in vol.items()})
        touched = vol["weight"] != before
        assert 0 < touched.sum() < touched.size and (depth == 0).any()
    # what the poses are there for
    assert (frames[1][0] > DEPTH_TRUNC).any() and ((frames[1][0] > 0) & (frames[1][0] <= DEPTH_TRUNC)).any()
    m = frames[2][2].astype(np.float64)
    zc = m[2, 0] * px[None, None, :] + m[2, 1] * py[None, :, None] + m[2, 2] * pz[:, None, None] + m[2, 3]
    assert (zc < 0).sum() > 1000 and (zc > 0).sum() > 1000
    m = frames[0][2].astype(np.float64)
    uf = (px[None, None, :] * FX) / pz[:, None, None] + CX + 0.5
    assert (uf < 0).any() and (uf >= W).any()
    assert states[2]["weight"].max() == 3 and (states[2]["weight"] == 0).any()
    return frames, states


def _volume(dev, dims=DIMS, origin=ORIGIN, length=L, trunc=TRUNC):
    import dqo_eval
    return dqo_eval.TsdfVolume(origin, float(length), dims, float(trunc), dev)


def _same(vol, state, what):
    import torch
    torch.cuda.synchronize()
    for name in ("tsdf", "weight", "color"):
        got, want = getattr(vol, name).cpu().numpy(), state[name]
        assert got.dtype == np.float32 and got.shape == want.shape
        bad = got.view(np.uint32) != want.view(np.uint32)
        assert not bad.any(), (what, name, int(bad.sum()), got[bad][:4], want[bad][:4])


def _dev():
    import torch
    return torch.device("cuda")


def test_integrate_equals_the_oracle_after_every_frame():
    import torch
    dev = _dev()
    frames, states = scene()
    vol = _volume(dev)
    _same(vol, O.clear(DIMS), "cleared")
    assert vol.counts() == dict(vertices=0, faces=0, vertices_dropped=0, faces_dropped=0, frames=0, frames_skipped=0)
    t = lambda a: torch.from_numpy(a).to(dev)
    for k, (depth, color, w2c) in enumerate(frames):
        # (K as four numbers, then as a matrix; depth as [H,W], then as [1,H,W])
        K = (FX, FY, CX, CY) if k != 1 else [[FX, 0, CX], [0, FY, CY], [0, 0, 1]]
        vol.integrate(t(depth) if k != 2 else t(depth)[None], t(color), K, t(w2c), depth_trunc=DEPTH_TRUNC)
        _same(vol, states[k], f"frame {k}")
    assert vol.counts()["frames"] == 3 and vol.counts()["frames_skipped"] == 0
    # a frame whose render outgrew its context changes nothing but header[5]
    over = torch.zeros((8,), dtype=torch.int32, device=dev)
    over[2] = 1  # DqoRastHeader.overflow
    vol.integrate(t(frames[0][0]), t(frames[0][1]), (FX, FY, CX, CY), t(frames[0][2]), depth_trunc=DEPTH_TRUNC, render_header=over)
    _same(vol, states[2], "overflowed frame")
    assert vol.counts()["frames"] == 3 and vol.counts()["frames_skipped"] == 1
    fine = torch.zeros((8,), dtype=torch.int32, device=dev)
    # depth_trunc below every depth, and a frame of d = 0: nothing changes; both count as frames
    vol.integrate(t(frames[0][0]), t(frames[0][1]), (FX, FY, CX, CY), t(frames[0][2]), depth_trunc=0.05, render_header=fine)
    vol.integrate(t(0 * frames[0][0]), t(frames[0][1]), (FX, FY, CX, CY), t(frames[0][2]), depth_trunc=DEPTH_TRUNC)
    _same(vol, states[2], "nothing to integrate")
    assert vol.counts()["frames"] == 5
    vol.clear()
    _same(vol, O.clear(DIMS), "cleared again")
    assert vol.counts()["frames"] == 0 and vol.counts()["frames_skipped"] == 0


def _load(vol, tsdf, weight, color):
    import torch
    vol.tsdf.copy_(torch.from_numpy(tsdf))
    vol.weight.copy_(torch.from_numpy(weight))
    vol.color.copy_(torch.from_numpy(color))


def _mesh_bytes(m, nv, nf):
    import torch
    torch.cuda.synchronize()
    return (m["vertices"][:nv].cpu().numpy().tobytes(), m["colors"][:nv].cpu().numpy().tobytes(), m["faces"][:nf].cpu().numpy().tobytes())


def _assert_mesh(m, want, what):
    nv, nf = int(want["header"][0]), int(want["header"][1])
    assert m["header"][:4].cpu().numpy().tolist() == want["header"].tolist(), what
    got = _mesh_bytes(m, nv, nf)
    assert got[0] == want["vertices"].tobytes(), (what, "vertices")
    assert got[1] == want["colors"].tobytes(), (what, "colors")
    assert got[2] == want["faces"].tobytes(), (what, "faces")


@functools.lru_cache(maxsize=2)
def _oracle_mesh(which):
    if which == "sphere":
        origin, length, tsdf, weight, color = O.sphere_volume()
        return (24, 24, 24), origin, length, tsdf, weight, color, O.extract(tsdf, weight, color, origin, length)
    s = scene()[1][2]
    return DIMS, ORIGIN, L, s["tsdf"], s["weight"], s["color"], O.extract(s["tsdf"], s["weight"], s["color"], ORIGIN, L)


@pytest.mark.parametrize("which", ["sphere", "integrated"])
def test_extract_equals_the_oracle(which):
    import torch
    dev = _dev()
    dims, origin, length, tsdf, weight, color, want = _oracle_mesh(which)
    V, F = len(want["vertices"]), len(want["faces"])
    assert V > 1000 and F > 1000
    if which == "integrated":  # an open mesh: the volume has unobserved parts
        assert (weight == 0).any() and len(np.unique(want["faces"])) == V
    vol = _volume(dev, dims, origin, length)
    _load(vol, tsdf, weight, color)
    m = vol.extract(V + 13, F + 7)
    _assert_mesh(m, want, which)
    assert m["header"] is vol.header and vol.counts()["vertices"] == V and vol.counts()["faces"] == F
    first = _mesh_bytes(m, V, F)
    before = torch.cuda.memory_allocated()
    again = vol.extract(V + 13, F + 7)
    assert again is m and torch.cuda.memory_allocated() == before  # (after the first call of a shape nothing is allocated)
    assert _mesh_bytes(again, V, F) == first  # two runs: identical bytes
    # exact capacities, and a caller's buffers
    mine = dict(vertices=torch.empty((V, 3), device=dev), colors=torch.empty((V, 3), device=dev),
                faces=torch.empty((F, 3), dtype=torch.int32, device=dev))
    assert vol.extract(V, F, out=mine) is mine
    _assert_mesh(mine, want, which + " exact")


@pytest.mark.parametrize("cut", ["faces", "vertices", "both", "zero"])
def test_extract_capacities(cut):
    """Capacities below the need: the written prefix is the oracle's, the dropped counts are exact, the words behind are untouched."""
    import torch
    dev = _dev()
    dims, origin, length, tsdf, weight, color, full = _oracle_mesh("sphere")
    V, F = len(full["vertices"]), len(full["faces"])
    cap_v, cap_f = dict(faces=(V, F - 1234), vertices=(V - 777, F), both=(V - 300, 2000), zero=(0, 0))[cut]
    want = O.extract(tsdf, weight, color, origin, length, cap_vertices=cap_v, cap_faces=cap_f)
    if cut in ("vertices", "both"):
        assert want["header"][2] == V - cap_v
    if cut == "vertices":
        assert 0 < want["header"][3] < F and want["header"][1] < cap_f  # faces left because their vertex did
    vol = _volume(dev, dims, origin, length)
    _load(vol, tsdf, weight, color)
    GUARD, guard_f, guard_i = 64, 12345.5, -77
    fv = torch.full((cap_v * 3 + GUARD,), guard_f, device=dev)
    fc = torch.full((cap_v * 3 + GUARD,), guard_f, device=dev)
    ff = torch.full((cap_f * 3 + GUARD,), guard_i, dtype=torch.int32, device=dev)
    out = dict(vertices=fv[:cap_v * 3].view(cap_v, 3), colors=fc[:cap_v * 3].view(cap_v, 3), faces=ff[:cap_f * 3].view(cap_f, 3))
    m = vol.extract(cap_v, cap_f, out=out)
    _assert_mesh(m, want, cut)
    nv, nf = int(want["header"][0]), int(want["header"][1])
    assert (fv[3 * nv:] == guard_f).all() and (fc[3 * nv:] == guard_f).all() and (ff[3 * nf:] == guard_i).all()
    c = vol.counts()
    assert (c["vertices"], c["faces"], c["vertices_dropped"], c["faces_dropped"]) == tuple(want["header"].tolist())
    assert c["vertices"] + c["vertices_dropped"] == V and c["faces"] + c["faces_dropped"] == F


@functools.lru_cache(maxsize=1)
def _map_scene():
    """An 8 k Gaussian frustum cloud at 160 x 120 seen from three cameras (the scene of tests/test_gpu_eval.py's kind)."""
    import torch
    from dqo_harness import mapping, scenes
    dev = torch.device("cuda")
    cams = [scenes.Camera(160, 120, 131.25, 131.25, 79.5, 59.5, scenes.rot_yx(yaw, pitch), np.array(t))
            for yaw, pitch, t in ((7.0, -3.0, [0.05, -0.02, 0.1]), (3.0, 1.0, [-0.1, 0.03, 0.2]), (11.0, -6.0, [0.15, -0.05, 0.0]))]
    scene_ = scenes.frustum_cloud(17, 8000, cams[0])
    return dev, scene_, cams, [mapping.make_settings(c, dev) for c in cams]


def test_make_mesh_equals_integrate_by_hand_and_then_allocates_nothing():
    import torch
    import dqo_eval
    from dqo_harness.fused_mapping import FusedMapper
    dev, scene_, cams, settings = _map_scene()
    fm = FusedMapper(scene_, settings[0], dev)
    box = dict(origin=(-1.5, -1.5, 0.2), voxel_length=0.0625, dims=(48, 47, 50), sdf_trunc=0.25, device=dev)
    vol = dqo_eval.TsdfVolume(**box)
    frames = [None, settings[1], settings[2]]
    assert fm.make_mesh(frames, vol, depth_trunc=4.0) is vol
    torch.cuda.synchronize()
    assert not fm.maintain_overflowed()
    got = {k: getattr(vol, k).clone() for k in ("tsdf", "weight", "color")}
    assert vol.counts()["frames"] == 3 and vol.counts()["frames_skipped"] == 0
    # by hand: _maintain_render's own outputs for the same cameras
    hand = dqo_eval.TsdfVolume(**box)
    for st, cam in zip(settings, cams):
        c = fm._maintain_render(st)
        w2c = st.viewmatrix.reshape(4, 4).t().contiguous()
        assert np.array_equal(w2c.cpu().numpy(), np.float32(cam.Rt))  # the world-to-camera matrix, row major
        Wd, Hd = 160, 120
        K = (Wd / (2.0 * float(st.tanfovx)), Hd / (2.0 * float(st.tanfovy)), float(st.cx), float(st.cy))
        assert abs(K[0] - 131.25) < 1e-9 * 131.25 + 1e-6 and (K[2], K[3]) == (79.5, 59.5)
        hand.integrate(c.out[1], c.out[0], K, w2c, depth_trunc=4.0, render_header=c.geom)
    torch.cuda.synchronize()
    for k in got:
        assert torch.equal(got[k].view(torch.int32), getattr(hand, k).view(torch.int32)), k
    assert (got["weight"] > 0).any() and (got["weight"] == 0).any()
    # the mesh is there
    m = vol.extract(400000, 800000)
    n = vol.counts()
    assert n["vertices"] > 100 and n["faces"] > 100 and n["vertices_dropped"] == 0 and n["faces_dropped"] == 0
    faces = m["faces"][:n["faces"]].cpu().numpy()
    assert faces.min() == 0 and faces.max() == n["vertices"] - 1 and len(np.unique(faces)) == n["vertices"]
    verts = m["vertices"][:n["vertices"]].cpu().numpy()
    assert np.isfinite(verts).all() and (verts >= np.array(box["origin"], np.float32)).all()
    assert (verts <= np.array(box["origin"], np.float32) + 0.0625 * np.array(box["dims"], np.float32)).all()
    cols = m["colors"][:n["vertices"]].cpu().numpy()
    assert np.isfinite(cols).all()
    # a second call: no allocation, no host read
    vol.clear()
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    torch.cuda.set_sync_debug_mode("error")
    try:
        fm.make_mesh(frames, vol, depth_trunc=4.0)
        vol.extract(400000, 800000)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.cuda.memory_allocated() == before
    torch.cuda.synchronize()
    for k in got:
        assert torch.equal(got[k].view(torch.int32), getattr(vol, k).view(torch.int32)), k
    assert vol.counts()["vertices"] == n["vertices"] and vol.counts()["faces"] == n["faces"]


def test_a_sharded_mapper_refuses():
    import dqo_eval
    from dqo_harness.fused_mapping import FusedMapper
    dev, scene_, cams, settings = _map_scene()
    fm = FusedMapper(scene_, settings[0], dev, attach_count_reducer=lambda n: n)
    vol = dqo_eval.TsdfVolume((-1.0, -1.0, 0.2), 0.25, (8, 8, 8), 0.5, dev)
    with pytest.raises(NotImplementedError, match="sharded"):
        fm.make_mesh([None], vol)
