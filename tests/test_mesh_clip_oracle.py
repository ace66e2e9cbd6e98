"""The numpy restatements of dqo_mesh_render_depth_clip and dqo_mesh_cull_faces (tests/mesh_clip_oracle.py) against what can be said
without them: analytic depths of a cube seen from inside and of a wall that crosses the near plane, the plain render's oracle wherever no
pair crosses, and a face cull counted by hand.  No GPU."""
import numpy as np
import pytest

import mesh_clip_oracle as C
import mesh_render_oracle as R

REL = 2e-5  # test_cube_against_the_analytic_ray_box_depth's bound
K, W, H = (30.0, 31.0, 17.25, 14.5), 37, 29


def inside_views(count=12, seed=1):
    """`count` seeded cameras within 0.3 of the unit cube's centre, looking anywhere."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        eye = rng.uniform(-0.3, 0.3, size=3) / np.sqrt(3.0)
        d = rng.normal(size=3)
        out.append(R.look_at(eye, eye + d / np.linalg.norm(d)))
    return np.stack(out)


@pytest.mark.parametrize("near", [0.0, 0.05])
def test_cube_from_inside_has_no_hole_and_the_analytic_exit_depth(near):
    v, f = R.cube_mesh()
    views = inside_views()
    r = C.render(v, f, views, K, W, H, near=near)
    crossing = r["crossing"].sum(1)
    assert ((crossing >= 8) & (crossing <= 10)).all(), crossing  # of a view's 12 pairs
    assert r["header"][3] == crossing.sum() and r["header"][2] + r["header"][4] <= 12 * len(views)
    assert (r["face_index"] >= 0).all() and (r["depth"] > 0).all()  # every pixel is hit
    worst = 0.0
    for k in range(len(views)):
        want = C.ray_box_exit_depth(views[k], K, W, H, R.CUBE_LO, R.CUBE_HI)
        worst = max(worst, float(np.abs(r["depth"][k].astype(np.float64) - want).max() / want.min()))
        assert (np.abs(r["depth"][k].astype(np.float64) - want) <= REL * want).all(), k
    print("cube from inside: worst error / smallest depth", worst)


def test_wall_quad_is_clipped_not_dropped():
    views = C.wall_views()
    shown = []
    for k in range(len(views)):
        one = views[k:k + 1]
        plain = R.render(C.WALL_VERTICES, C.WALL_FACES, one, C.WALL_K, C.WALL_W, C.WALL_H)
        assert plain["header"].tolist() == [1, 0, 0, 2, 0, 0, 0, 0] and not plain["depth"].any()  # today's rule: an empty image
        r = C.render(C.WALL_VERTICES, C.WALL_FACES, one, C.WALL_K, C.WALL_W, C.WALL_H)
        assert r["header"][3] == 2 and r["header"][4] == 0  # pairs_near_clipped; [2] leaves out a pair whose box misses the image
        want = C.ray_quad_depth(one[0], C.WALL_K, C.WALL_W, C.WALL_H)
        assert want.any()
        assert ((r["depth"][0] > 0) == (want > 0)).all(), k  # the analytic hit set: nothing missing on the diagonal, nothing behind
        hit = want > 0
        err = np.abs(r["depth"][0].astype(np.float64) - want)[hit] / want[hit]
        print("wall view", k, "pixels hit", int(hit.sum()), "worst relative error", float(err.max()))
        assert (err <= REL).all(), (k, float(err.max()))
        assert r["header"][6] == hit.sum()
        shown.append(set(np.unique(r["face_index"][0][hit]).tolist()))
        assert r["header"][2] >= len(shown[-1])
    assert shown[2] == {0, 1}, shown  # the third view shows both triangles: their diagonal runs through its image, and no pixel on it is missing


def test_wall_seen_frontally_is_the_plain_render():
    front = R.look_at((2.0, 1.0, -3.0), (2.0, 1.0, 1.0))[None]
    a = R.render(C.WALL_VERTICES, C.WALL_FACES, front, C.WALL_K, C.WALL_W, C.WALL_H)
    b = C.render(C.WALL_VERTICES, C.WALL_FACES, front, C.WALL_K, C.WALL_W, C.WALL_H)
    assert b["header"][3] == 0 and not b["crossing"].any()
    for name in ("depth", "face_index", "header", "keys"):
        assert a[name].tobytes() == b[name].tobytes(), name


def test_mixed_scene_differs_from_the_plain_render_only_where_a_crossing_face_wins():
    s = R.mixed_scene()
    a = R.render(s["vertices"], s["faces"], s["w2c"], s["K"], s["W"], s["H"], near=s["near"])
    b = C.render(s["vertices"], s["faces"], s["w2c"], s["K"], s["W"], s["H"], near=s["near"])
    assert b["header"][3] == a["header"][3] > 0 and b["header"][[0, 1]].tolist() == a["header"][[0, 1]].tolist()
    won = np.zeros(b["face_index"].shape, bool)
    for k in range(len(s["w2c"])):
        won[k] = np.isin(b["face_index"][k], np.nonzero(b["crossing"][k])[0])
    assert won.any()  # the crossing triangles have hits now
    assert (a["keys"][~won] == b["keys"][~won]).all() and (b["keys"][won] < a["keys"][won]).all()
    assert b["header"][2] > a["header"][2]


def test_shuffled_faces_give_the_same_depth():
    v, f = R.cube_mesh()
    views = inside_views(4, seed=9)
    a = C.render(v, f, views, K, W, H, near=0.05)
    perm = np.random.default_rng(3).permutation(len(f))
    b = C.render(v, f[perm], views, K, W, H, near=0.05)
    assert a["depth"].tobytes() == b["depth"].tobytes() and a["header"].tolist() == b["header"].tolist()
    same_depth_elsewhere = perm[b["face_index"]] != a["face_index"]  # (two faces may give one depth on their shared edge)
    assert same_depth_elsewhere.mean() < 0.05


def test_face_cull_by_hand():
    verts = np.arange(9 * 3, dtype=np.float32).reshape(9, 3)
    cols = verts[::-1].copy()
    # face 3 has a bad index; vertex 3 is named by face 2 alone
    faces = np.array([[0, 1, 2], [2, 8, 4], [4, 3, 6], [1, 9, 2], [5, 6, 7], [0, 2, 4]], np.int32)
    fi = np.full((2, 3, 4), -1, np.int32)
    fi[0] = [[0, 0, 1, 1], [1, 2, 3, 3], [6, -1, 99, 4]]  # 3: a bad face's id; 6, 99, -1: never an index
    fi[1] = [[5, 5, 5, 5], [5, 5, 0, -7], [4, 4, 1 << 30, -(1 << 31)]]
    rd = np.full((2, 3, 4), 2.0, np.float32)
    r = C.cull_faces(verts, cols, faces, fi, rd)
    assert r["face_pixels"].tolist() == [3, 3, 1, 0, 3, 6]
    assert r["header"].tolist() == [9, 5, 5, 2, 1, 0, 0, 16]
    assert r["faces"].tolist() == [[0, 1, 2], [2, 8, 4], [4, 3, 6], [5, 6, 7], [0, 2, 4]] and r["vertices"].tobytes() == verts.tobytes()
    r = C.cull_faces(verts, cols, faces, fi, rd, min_pixels=3)
    assert r["header"].tolist() == [8, 4, 5, 2, 1, 1, 1, 16]  # face 2 goes with its one pixel, and vertex 3 with it
    kept = [0, 1, 4, 5]
    named = sorted(set(faces[kept].ravel().tolist()))
    remap = {v: i for i, v in enumerate(named)}
    assert r["faces"].tolist() == [[remap[a] for a in faces[g]] for g in kept]
    assert r["vertices"].tobytes() == verts[named].tobytes() and r["colors"].tobytes() == cols[named].tobytes()
    r = C.cull_faces(verts, None, faces, fi, rd, view_keep=[1, 0], min_pixels=4)
    assert r["face_pixels"].tolist() == [2, 3, 1, 0, 1, 0] and r["header"].tolist() == [0, 0, 4, 1, 1, 5, 9, 7] and r["colors"] is None
    # occlusion: the frames' depth lies nearer than the render minus eps in view 1, and has holes and far pixels in view 0
    depth = np.full((2, 3, 4), 2.0, np.float32)
    depth[1] = 1.9
    depth[0, 0, 0], depth[0, 0, 2], depth[0, 1, 0] = 0.0, 7.0, 1.97
    r = C.cull_faces(verts, cols, faces, fi, rd, depth=depth, eps=0.03, depth_trunc=5.0)
    assert r["face_pixels"].tolist() == [1, 2, 1, 0, 1, 0]  # (0,0,0): no depth; (0,0,2): beyond the truncation; (0,1,0): 2.0 <= 1.97 + 0.03
    assert r["header"].tolist()[1:6] == [4, 4, 2, 1, 1] and r["header"][7] == 5
