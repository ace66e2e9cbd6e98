"""CPU: the floater-pruning oracle (tests/prune_oracle.py) itself — the geometry of the four virtual cameras, the deletion rule on hand-made
maps, and a small scene with scripted fates rendered by the CPU oracle rasteriser at the oracle's cameras.  No GPU."""
import functools

import numpy as np
import pytest
import torch

import lifecycle_cases as lc
import prune_oracle as po


# ---- geometry -----------------------------------------------------------------------------------------------------------------------------
def _random_pose(seed):
    from dqo_harness import scenes
    rng = np.random.default_rng(seed)
    cam = scenes.Camera(50, 36, 40.0, 42.0, 24.5, 17.5, scenes.rot_yx(float(rng.uniform(-90, 90)), float(rng.uniform(-40, 40))), rng.uniform(-3, 3, 3))
    depth = rng.uniform(0.4, 5.0, (36, 50)).astype(np.float32)
    return cam, depth, int(rng.integers(0, 36 * 50))


@pytest.mark.parametrize("seed", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("theta", [3.0, 10.0])
def test_the_virtual_cameras_turn_about_the_focal_point(seed, theta):
    cam, depth, pixel = _random_pose(seed)
    # (the pose in double, orthonormal to 1e-16: the camera's float32 view matrix is orthonormal to 1e-7 only, and so are its R_k)
    v = po.virtual_cameras(cam.Rt.T.copy(), cam.projection_matrix, depth, pixel, *po.host_cos_sin(theta))
    Rw, T, focal, offset = v["Rw"], v["T0"], v["focal64"], v["offset"]
    assert np.array_equal(Rw, cam.Rw2c) and np.array_equal(T, cam.t)  # camera_R = frame.R.transpose(0, 1), camera_T = frame.T
    d = -np.float64(depth.reshape(-1)[pixel])
    assert v["d"] == d and np.array_equal(focal, T + d * Rw[:, 2]) and np.array_equal(offset, T - focal)
    c, s = po.host_cos_sin(theta)
    for k in range(4):
        A = np.array(po.rotation_matrix("y" if k < 2 else "x", np.float64(c), np.float64(s if k % 2 == 0 else -s)))
        Rk, Tk = v["R"][k], v["T"][k]
        assert np.abs(Rk - A @ Rw).max() < 1e-12
        assert np.abs(Rk.T @ Rk - np.eye(3)).max() < 1e-12 and np.abs(Rk @ Rk.T - np.eye(3)).max() < 1e-12  # R_k is orthonormal
        assert abs(np.linalg.norm(Tk - focal) - np.linalg.norm(offset)) < 1e-12  # A_k fixes the focal point
        rel = Rk @ Rw.T
        ang = np.degrees(np.arccos(np.clip((np.trace(rel) - 1) / 2, -1, 1)))
        assert abs(ang - theta) < 1e-9, (k, ang)
        # the camera tables: R_k as it stands, T_k in the last row, the last column (0, 0, 0, 1); projmatrix = viewmatrix @ projection
        V = v["viewmatrix"][k]
        assert np.array_equal(V[:3, :3], Rk.astype(np.float32)) and np.array_equal(V[3, :3], Tk.astype(np.float32))
        assert np.array_equal(V[:, 3], np.array([0, 0, 0, 1], np.float32))
        V64 = np.zeros((4, 4))
        V64[:3, :3], V64[3, :3], V64[3, 3] = Rk, Tk, 1.0
        want = V64 @ cam.projection_matrix.astype(np.float64)
        assert np.allclose(v["projmatrix"][k], want, rtol=1e-6, atol=1e-7)
    # the pairs are mirror images: Ry(+t) Ry(-t) = 1
    assert np.abs(v["R"][0] @ Rw.T @ v["R"][1] @ Rw.T - np.eye(3)).max() < 1e-12


def test_an_orthonormal_pose_gives_orthonormal_cameras():
    """With a rotation that is orthonormal in double (a signed permutation is exact in float32) each R_k is orthonormal to 1e-12."""
    vm = np.zeros((4, 4), np.float32)
    vm[:3, :3] = np.array([[0, 0, 1], [-1, 0, 0], [0, -1, 0]], np.float32)
    vm[3, :3], vm[3, 3] = (0.25, -1.5, 2.0), 1.0
    depth = np.full((4, 6), 1.75, np.float32)
    v = po.virtual_cameras(vm, np.eye(4, dtype=np.float32), depth, 5, *po.host_cos_sin(3.0))
    for k in range(4):
        assert np.abs(v["R"][k].T @ v["R"][k] - np.eye(3)).max() < 1e-12
        assert abs(np.linalg.norm(v["T"][k] - v["focal64"]) - np.linalg.norm(v["offset"])) < 1e-12
        assert abs(np.linalg.norm(v["offset"]) - 1.75) < 1e-12


def test_zero_depth_puts_the_focal_point_one_unit_away():
    cam, depth, pixel = _random_pose(7)
    depth.reshape(-1)[pixel] = 0.0
    v = po.virtual_cameras(cam.world_view_transform, cam.projection_matrix, depth, pixel, *po.host_cos_sin(3.0))
    assert v["d"] == -1.0 and np.array_equal(v["focal64"], v["T0"] + np.float64(-1.0) * v["Rw"][:, 2])


def test_the_centre_pixel():
    H, W = 36, 50
    assert po.centre_pixel(24.5, 17.5, H, W) == (24, 17)  # the reference: row int(cx), column int(cy)
    assert po.centre_pixel(24.5, 17.5, H, W, "principal") == (17, 24)  # the intent: row int(cy), column int(cx)
    assert po.centre_pixel(35.9, 49.9, H, W) == (35, 49)
    with pytest.raises(IndexError):
        po.centre_pixel(36.0, 17.5, H, W)  # int(cx) >= H
    assert po.centre_pixel(36.0, 17.5, H, W, "principal") == (17, 36)
    with pytest.raises(IndexError):
        po.centre_pixel(24.5, 50.0, H, W)


# ---- the rule -----------------------------------------------------------------------------------------------------------------------------
def _map(seed=3, **kw):
    case = lc.make_case(seed, **kw)
    state = case["state"]
    P = int(state["xyz"].shape[0])
    rng = np.random.default_rng(seed + 50)
    alive = state["alive"].numpy().astype(bool)
    state["frame_id"] = torch.from_numpy(np.where(alive, rng.integers(1, 9, P), 0).astype(np.int32))
    touched = torch.from_numpy(((rng.random(P) < 0.4) * rng.integers(1, 90, P)).astype(np.int64))
    return state, touched, case["kw"]["park"]


def _check(state, touched, window, r, skipped=False):
    lo, hi = window
    alive, stable, fid = state["alive"].bool(), state["stable"].bool(), state["frame_id"]
    in_window = alive & (fid > lo) & (fid <= hi)
    gone = in_window & (touched == 0) & (not skipped)
    assert r["stats"] == [int(in_window.sum()), int((gone & ~stable).sum()), int((gone & stable).sum()), r["stats"][3], int(skipped),
                          int(alive.sum()) - int(gone.sum()), 0, 0]
    out = r["state"]
    for k, v in state.items():
        assert torch.equal(out[k][~gone], v[~gone]), k  # every other row keeps every bit
    assert torch.equal(out["xyz"][gone], torch.as_tensor(lc.PARK).expand(int(gone.sum()), 3))
    for k, v in po.FREED.items():
        assert bool((out[k][gone] == v).all()), k
    f = lambda name: r["fate"] == po.FATES.index(name)
    assert torch.equal(f("spare"), ~alive) and torch.equal(f("deleted_unstable"), gone & ~stable) and torch.equal(f("deleted_stable"), gone & stable)
    assert torch.equal(f("outside_window"), alive & ~in_window)
    assert torch.equal(f("kept_skipped" if skipped else "kept_touched"), in_window & ~gone)
    return gone


def test_the_rule_on_hand_made_maps():
    state, touched, park = _map()
    # one id: (4, 5] is frame 5 alone — the reference's one-keyframe form (uid - 1, uid]
    gone = _check(state, touched, (4, 5), po.prune_oracle(state, touched, (4, 5), park))
    assert bool((state["frame_id"][gone] == 5).all()) and 0 < int(gone.sum())
    assert bool(state["stable"][gone].bool().any()) and bool((~state["stable"][gone].bool()).any())  # rows of both clouds
    # empty window
    r = po.prune_oracle(state, touched, (5, 5), park)
    assert not bool(_check(state, touched, (5, 5), r).any()) and r["stats"][:3] == [0, 0, 0]
    # a window covering everything: every untouched Gaussian leaves, spare rows stay spare rows
    gone = _check(state, touched, (0, 8), po.prune_oracle(state, touched, (0, 8), park))
    assert torch.equal(gone, state["alive"].bool() & (touched == 0))
    # boundaries: lo is outside, hi inside
    gone = _check(state, touched, (2, 4), po.prune_oracle(state, touched, (2, 4), park))
    assert set(state["frame_id"][gone].tolist()) == {3, 4}
    # skipped: some render was invalid
    r = po.prune_oracle(state, touched, (0, 8), park, invalid_renders=1, valid_renders=3)
    assert not bool(_check(state, touched, (0, 8), r, skipped=True).any()) and r["stats"][3:5] == [3, 1]
    for k, v in state.items():
        assert torch.equal(r["state"][k], v), k


@pytest.mark.parametrize("kw", [dict(n_alive=1, n_spare=0), dict(n_alive=0, n_spare=64)], ids=["one_row", "all_spare"])
def test_the_rule_on_degenerate_maps(kw):
    state, touched, park = _map(9, **kw)
    touched = torch.zeros_like(touched)
    r = po.prune_oracle(state, touched, (0, 8), park)
    _check(state, touched, (0, 8), r)
    assert r["stats"][1] + r["stats"][2] == kw["n_alive"] and r["stats"][5] == 0


# ---- scripted fates on the CPU oracle rasteriser ------------------------------------------------------------------------------------------
SCENE_H, SCENE_W = 48, 64
SCENE_WINDOW = (2, 3)
NAMED = ("front", "front_b", "behind", "outside", "masked", "hidden_outside_window")


def _scene():
    """(camera, scene dict, frame_id, named rows, tile mask, depth map): an opaque wall of 21 x 17 surfels at z = 2 in front of a camera
    that is slightly turned and shifted, and six named surfels.  The wall was added before the window; the named rows in it, but one."""
    from dqo_harness import scenes
    cam = scenes.Camera(SCENE_W, SCENE_H, 60.0, 60.0, 31.5, 23.5, scenes.rot_yx(4.0, -2.0), np.array([0.1, -0.05, 0.2]))
    to_world = lambda p: (np.asarray(p, np.float64) - cam.t) @ cam.Rw2c  # camera -> world: Rw2c^T (p - t)
    gx, gy = np.meshgrid(np.linspace(-1.6, 1.6, 21), np.linspace(-1.28, 1.28, 17))
    wall = np.stack([gx.ravel(), gy.ravel(), np.full(gx.size, 2.0)], 1)
    named_c = dict(front=(0.10, 0.05, 1.0), front_b=(-0.35, -0.2, 1.4), behind=(0.0, 0.1, 3.0), outside=(8.0, 0.0, 1.0), masked=(-0.3, 0.5, 1.8),
                   hidden_outside_window=(0.3, -0.2, 3.0))
    n_wall = wall.shape[0]
    xyz = np.concatenate([wall, np.array([named_c[k] for k in NAMED])])
    P = xyz.shape[0]
    named = {k: n_wall + i for i, k in enumerate(NAMED)}
    scales = np.tile(np.array([0.12, 0.12, 0.01]), (P, 1))
    opacity = np.full((P, 1), 0.99)
    for k, s, o in (("front", 0.03, 0.4), ("front_b", 0.04, 0.3), ("behind", 0.05, 0.9), ("outside", 0.05, 0.9), ("masked", 0.015, 0.4),
                    ("hidden_outside_window", 0.05, 0.9)):
        scales[named[k]], opacity[named[k]] = (s, s, 0.1 * s), o
    # the surfels face the camera: world rotation = Rw2c^T as a quaternion (r, x, y, z)
    Rm = cam.Rw2c.T
    r = np.sqrt(1.0 + np.trace(Rm)) / 2
    q = np.array([r, (Rm[2, 1] - Rm[1, 2]) / (4 * r), (Rm[0, 2] - Rm[2, 0]) / (4 * r), (Rm[1, 0] - Rm[0, 1]) / (4 * r)])
    shs = np.zeros((P, 16, 3))
    shs[:, 0] = np.random.default_rng(5).uniform(-1, 1, (P, 3))
    sc = dict(xyz=to_world(xyz).astype(np.float32), opacity=opacity.astype(np.float32), scales=scales.astype(np.float32),
              rotations=np.tile(q, (P, 1)).astype(np.float32), shs=shs.astype(np.float32))
    frame_id = np.full(P, 1, np.int32)
    for k in NAMED:
        frame_id[named[k]] = 3
    frame_id[named["hidden_outside_window"]] = 1
    tile_mask = np.ones(((SCENE_H + 15) // 16, (SCENE_W + 15) // 16), np.int32)
    tile_mask[2] = 0  # the image band y in [32, 48)
    depth = np.full((SCENE_H, SCENE_W), 2.0, np.float32)
    return cam, sc, frame_id, named, tile_mask, depth


def _at(cam, view, proj):
    """The camera as frame.update(R_k, T_k) leaves it: new transforms, the old camera_center (Camera.update never refreshes it)."""
    import copy
    c = copy.copy(cam)
    c.world_view_transform, c.full_proj_transform = view, proj
    return c


def _render_views(ol, cam, cams, sc, tile_mask, dtype, rows=None):
    import util_rast as U
    if rows is not None:
        sc = {k: v[rows] for k, v in sc.items()}
    out = []
    for k in range(4):
        _, res, _ = U.run_oracle(ol, _at(cam, cams["viewmatrix"][k], cams["projmatrix"][k]), sc, tile_mask=tile_mask, dtype=dtype)
        out.append(res)
    return out


def test_scripted_fates_on_the_oracle_rasteriser(oracle):
    """The conditions the scene must meet (a scene that fails them is a bad fixture): float32 and float64 agree on `touched` for every
    row; every touched window row has at least 4 touching pixels in total; every untouched named row is untouched for its named reason
    — radius 0 in all four views, masked tiles only, or transmittance <= 0.25 in front of it at every pixel it covers.  Then the rule
    gives every named row its fate."""
    cam, sc, frame_id, named, tile_mask, depth = _scene()
    P = sc["xyz"].shape[0]
    row, col = po.centre_pixel(cam.cx, cam.cy, SCENE_H, SCENE_W)
    assert (row, col) == (31, 23)
    cams = po.virtual_cameras(cam.world_view_transform, cam.projection_matrix, depth, row * SCENE_W + col, *po.host_cos_sin(3.0))
    views = {dt: _render_views(oracle, cam, cams, sc, tile_mask, dt) for dt in (np.float32, np.float64)}
    total = {dt: sum(v["n_touched"].astype(np.int64) for v in views[dt]) for dt in views}
    touched = total[np.float32] > 0
    assert np.array_equal(touched, total[np.float64] > 0), np.flatnonzero(touched != (total[np.float64] > 0))
    in_window = (frame_id > SCENE_WINDOW[0]) & (frame_id <= SCENE_WINDOW[1])
    for dt in views:
        assert (total[dt][in_window & touched] >= 4).all(), total[dt][in_window & touched]
    assert touched[named["front"]] and touched[named["front_b"]] and touched[:P - len(NAMED)].any()
    for k in ("behind", "outside", "masked", "hidden_outside_window"):
        assert not touched[named[k]], k
    for dt in views:
        # outside all four frusta: no footprint in any view
        assert all(v["radii"][named["outside"]] == 0 for v in views[dt])
        # masked tiles only: it has a footprint, the unmasked views touch it, the masked ones do not
        assert all(v["radii"][named["masked"]] > 0 for v in views[dt])
        unmasked = _render_views(oracle, cam, cams, sc, None, dt)
        assert sum(int(v["n_touched"][named["masked"]]) for v in unmasked) >= 4
        for k in ("front", "front_b", "behind", "hidden_outside_window"):  # (the mask is not what decides the others)
            assert (sum(int(v["n_touched"][named[k]]) for v in unmasked) > 0) == bool(touched[named[k]]), k
        # behind the wall: where the row alone leaves a mark, the Gaussians in front of it leave a transmittance of at most 0.25
        for k in ("behind", "hidden_outside_window"):
            r = named[k]
            assert all(v["radii"][r] > 0 for v in views[dt]), k
            alone = _render_views(oracle, cam, cams, sc, tile_mask, dt, rows=[r])
            front = _render_views(oracle, cam, cams, sc, tile_mask, dt, rows=np.arange(P - len(NAMED)))  # the wall
            for a, f in zip(alone, front):
                covered = a["T_map"][0] < 1.0
                assert covered.sum() >= 4 and (f["T_map"][0][covered] <= 0.25).all(), (k, float(f["T_map"][0][covered].max()))
    # the rule
    alive = np.ones(P, np.uint8)
    state = dict(xyz=torch.from_numpy(sc["xyz"].copy()), opacity_raw=torch.zeros(P, 1), scaling_raw=torch.from_numpy(np.log(sc["scales"])),
                 confidence=torch.ones(P), alive=torch.from_numpy(alive), row_flags=torch.zeros(P, dtype=torch.uint8),
                 stable=torch.from_numpy((np.arange(P) % 2).astype(np.uint8)), add_tick=torch.full((P,), 4, dtype=torch.int32),
                 depth_error_counter=torch.zeros(P, dtype=torch.int32), color_error_counter=torch.zeros(P, dtype=torch.int32),
                 frame_id=torch.from_numpy(frame_id.copy()))
    r = po.prune_oracle(state, torch.from_numpy(total[np.float32]), SCENE_WINDOW, torch.from_numpy(lc.PARK))
    fate = {k: po.FATES[int(r["fate"][named[k]])] for k in NAMED}
    assert fate["front"] == fate["front_b"] == "kept_touched" and fate["hidden_outside_window"] == "outside_window"
    assert {fate["behind"], fate["outside"], fate["masked"]} <= {"deleted_unstable", "deleted_stable"}
    assert r["stats"] == [5, r["stats"][1], r["stats"][2], 4, 0, P - 3, 0, 0] and r["stats"][1] + r["stats"][2] == 3
    assert bool((r["fate"][:P - len(NAMED)] == po.FATES.index("outside_window")).all())  # the wall stays, touched or not
