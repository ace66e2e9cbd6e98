"""GPU: no operator writes behind the workspace its size query asks for.  Every operator whose workspace has more than one part is called
through the Python surface on a caller-owned buffer of exactly the queried bytes, zero, inside a larger one whose last 4 096 bytes hold
0xA5: the guard is untouched afterwards, and a second call on the workspace the first one left gives the same output bytes.  The
shapes are the smallest that use every part — capacities 257 / 513 above the device counts, 1 025 faces and 257 samples, a 5 x 4 x 3
volume, 33 x 17 images (MS-SSIM and LPIPS: their smallest sides).  No new behaviour: the test holds on the commit before the layouts
were unified as well.  (dqo_knn3 and dqo_knn3_query get their workspaces from their Python wrappers, never from a caller.)"""
import numpy as np
import pytest

import sample_cases as sc

pytestmark = pytest.mark.gpu

GUARD = 4096
CAP_V, CAP_F = 257, 513


def _guarded(need):
    """(the workspace to hand over: `need` zero bytes, the whole buffer: the guard behind them)"""
    import torch
    assert need > 0
    buf = torch.zeros((need + GUARD,), dtype=torch.uint8, device="cuda")
    buf[need:] = 0xA5
    return buf[:need], buf


def _bytes(x):
    import torch
    if torch.is_tensor(x):
        return [x.detach().contiguous().view(torch.uint8).clone()]
    if isinstance(x, dict):
        return [b for k in sorted(x) if torch.is_tensor(x[k]) for b in _bytes(x[k])]
    return [b for t in x if t is not None for b in _bytes(t)]


def _check(need, call):
    """call(workspace) -> the tensors it wrote: twice on one guarded workspace"""
    import torch
    ws, buf = _guarded(need)
    first = _bytes(call(ws))
    second = _bytes(call(ws))
    torch.cuda.synchronize()
    assert bool((buf[need:] == 0xA5).all()), "the guard behind the workspace was written"
    assert len(first) == len(second) > 0 and all(torch.equal(a, b) for a, b in zip(first, second))


def _mesh(colors):
    """Two components — a 10 x 10 sheet and a quad beside it — in buffers of CAP_V / CAP_F rows, the counts in a device header."""
    import torch
    g = np.stack(np.meshgrid(np.arange(10), np.arange(10), indexing="ij"), -1).reshape(-1, 2)
    v = np.concatenate([np.c_[g * 0.1 - 0.45, 2.0 + 0.03 * np.sin(g[:, :1] + g[:, 1:])], [[0.7, 0, 2], [0.8, 0, 2], [0.7, 0.1, 2], [0.8, 0.1, 2.1]]])
    q = np.array([[i * 10 + j, i * 10 + j + 1, i * 10 + j + 10, i * 10 + j + 11] for i in range(9) for j in range(9)] + [[100, 101, 102, 103]])
    f = np.concatenate([q[:, [0, 1, 2]], q[:, [1, 3, 2]]])
    V, F = len(v), len(f)
    assert V < CAP_V and F < CAP_F
    d = dict(vertices=torch.full((CAP_V, 3), float("nan"), device="cuda"), faces=torch.full((CAP_F, 3), 1 << 30, dtype=torch.int32, device="cuda"),
             header=torch.tensor([V, F, 0, 0, 0, 0, 0, 0], dtype=torch.int32, device="cuda"))
    d["vertices"][:V] = torch.tensor(v, dtype=torch.float32)
    d["faces"][:F] = torch.tensor(f, dtype=torch.int32)
    if colors:
        d["colors"] = torch.rand((CAP_V, 3), device="cuda", generator=torch.Generator("cuda").manual_seed(3))
    return d


def _mesh_need(op):
    import _dqo_native as N
    return getattr(N.lib(), f"dqo_mesh_{op}_workspace_bytes")(CAP_V, CAP_F)


@pytest.mark.parametrize("colors", [True, False], ids=["colours", "no_colours"])
@pytest.mark.parametrize("extra", [True, False], ids=["labels_views", "plain"])
def test_mesh_operators(colors, extra):
    import torch
    import dqo_eval as E
    mesh = _mesh(colors)
    _check(_mesh_need("components"), lambda ws: E.mesh_components(mesh, min_faces=3, want_labels=extra, workspace_buffer=ws))
    _check(_mesh_need("simplify"), lambda ws: E.mesh_simplify(mesh, 0.25, origin=(-1.0, -1.0, 1.0), workspace_buffer=ws))
    _check(_mesh_need("normals"), lambda ws: E.mesh_normals(mesh, workspace_buffer=ws)["normals"])
    w2c = torch.eye(4, device="cuda").reshape(1, 16).repeat(3, 1).contiguous()
    depth = torch.full((3, 17, 33), 2.02, device="cuda") if extra else None
    _check(_mesh_need("cull"), lambda ws: E.mesh_cull(mesh, w2c, (20.0, 20.0, 16.0, 8.0), 33, 17, depth=depth, min_corners=2, want_views=extra,
                                                      workspace_buffer=ws))

    def smooth(ws):  # (in place: every call starts from the same mesh)
        m = {k: v.clone() for k, v in mesh.items()}
        return E.mesh_smooth(m, 2, lam=0.5, mu=-0.53 if extra else None, workspace_buffer=ws)
    _check(_mesh_need("smooth"), smooth)


def test_mesh_samplers():
    import torch
    import _dqo_native as N
    import dqo_eval as E
    g = torch.Generator("cuda").manual_seed(5)
    F, count = 1025, 257
    v = torch.rand((600, 3), device="cuda", generator=g)
    f = torch.randint(0, 600, (F, 3), device="cuda", generator=g, dtype=torch.int32)
    need = N.lib().dqo_mesh_sample_workspace_bytes(F, count)
    assert need == N.lib().dqo_mesh_sample_counted_workspace_bytes(F, count)
    _check(need, lambda ws: E.sample_surface(v, f, count, seed=9, want_face_index=True, workspace_buffer=ws))
    mesh = dict(vertices=v, faces=f, header=torch.tensor([590, 1000], dtype=torch.int32, device="cuda"))
    _check(need, lambda ws: E.sample_surface_counted(mesh, count, seed=9, want_face_index=True, workspace_buffer=ws))


def test_tsdf_extract():
    import torch
    import _dqo_native as N
    import dqo_eval as E
    vol = E.TsdfVolume((-0.25, -0.2, 0.0), 0.1, (5, 4, 3), 0.3, "cuda")
    depth = torch.full((17, 33), 0.17, device="cuda")
    color = torch.rand((3, 17, 33), device="cuda", generator=torch.Generator("cuda").manual_seed(1))
    vol.integrate(depth, color, (8.0, 8.0, 16.0, 8.0), torch.eye(4, device="cuda").reshape(16).contiguous())

    def extract(ws):
        vol._ws = ws
        m = vol.extract(200, 400)
        return [m["vertices"], m["colors"], m["faces"], m["header"]]
    _check(N.lib().dqo_tsdf_workspace_bytes(5, 4, 3), extract)
    assert vol.counts()["frames"] == 1 and vol.counts()["faces"] > 0


def test_eval_picture_with_its_ssim_and_the_growth_sampler():
    import torch
    import _dqo_native as N
    import dqo_eval as E
    import dqo_mapgrowth as mg
    H, W = 17, 33
    g = torch.Generator("cuda").manual_seed(2)
    rnd = lambda *s: torch.rand(s, device="cuda", generator=g)
    render = dict(render=rnd(3, H, W), depth=rnd(1, H, W) + 0.5, depth_index_map=torch.randint(-1, 5, (1, H, W), device="cuda", generator=g, dtype=torch.int32))
    gt_color, gt_depth = rnd(3, H, W), rnd(1, H, W) + 0.5
    lib = N.lib()
    need = lib.dqo_eval_picture_workspace_bytes(W, H) + lib.dqo_map_ssim_workspace_bytes(W, H)
    assert need == E.workspace(W, H, "cuda").numel()
    _check(need, lambda ws: E.eval_picture(render, gt_color, gt_depth, 0.1, 5.0, workspace_buffer=ws))

    frame, model = sc.make_frame(H=H, W=W)
    cuda = lambda d: {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in d.items() if v is not None}
    f, m = cuda(frame), cuda(model)
    buffers = mg.sample_buffers(mg.sample_capacity(H, W, False, 300, 2.0, 0.3), 16, "cuda")
    for b in buffers.values():
        b.zero_()

    def sample(ws):
        _, header = mg.temp_points_init(f, m, buffers=buffers, workspace=ws, **dict(sc.SMALL, seed=2, tick=0))
        assert header["rows"] > 0
        return buffers
    _check(lib.dqo_growth_sample_workspace_bytes(W, H), sample)


def test_the_other_multi_part_workspaces():
    """MS-SSIM, LPIPS, the window masks, the exact 1-NN search and the two geometry tables"""
    import torch
    import _dqo_native as N
    import dqo_eval as E
    import dqo_tilemask as M
    lib = N.lib()
    g = torch.Generator("cuda").manual_seed(4)
    rnd = lambda *s: torch.rand(s, device="cuda", generator=g)
    a, b = rnd(3, 161, 161), rnd(3, 161, 161)
    _check(lib.dqo_eval_ms_ssim_workspace_bytes(161, 161), lambda ws: E.ms_ssim(a, b, workspace_buffer=ws))
    wts = E.LpipsWeights([rnd(co, ci, k, k) - 0.5 for ci, co, k, _, _ in E.LPIPS_NET], [rnd(co) - 0.5 for _, co, _, _, _ in E.LPIPS_NET],
                         [rnd(co) for _, co, _, _, _ in E.LPIPS_NET], "cuda")
    _check(lib.dqo_eval_lpips_workspace_bytes(31, 31), lambda ws: E.lpips(a[:, :31, :31], b[:, :31, :31], wts, workspace_buffer=ws))
    T_map = torch.where(rnd(17, 33) < 0.5, torch.ones((), device="cuda"), rnd(17, 33))
    need = lib.dqo_window_masks_workspace_bytes(33, 17)
    _check(need, lambda ws: M.window_masks(T_map, workspace=ws))
    small_a, small_b = a[:, :17, :33].contiguous(), b[:, :17, :33].contiguous()
    _check(need, lambda ws: M.window_masks(T_map, small_a, small_b, global_opt=True, sample_ratio=0.5, workspace=ws))
    gt, rec = rnd(300, 3), rnd(257, 3)
    gt_obj = torch.randint(-1, 3, (300,), device="cuda", generator=g, dtype=torch.int32)
    rec_obj = torch.randint(-1, 3, (257,), device="cuda", generator=g, dtype=torch.int32)
    _check(lib.dqo_nn1_workspace_bytes(257, 300), lambda ws: E.nearest(rec, gt, query_keep=rec_obj >= 0, workspace_buffer=ws))
    _check(lib.dqo_nn1_grouped_workspace_bytes(257, 300), lambda ws: E.nearest_grouped(rec, rec_obj, gt, gt_obj, workspace_buffer=ws))
    _check(lib.dqo_eval_pcd_workspace_bytes(300, 257), lambda ws: E.eval_pcd(gt, rec, (0.03, 0.1), gt_keep=gt_obj >= 0, workspace_buffer=ws))
    _check(lib.dqo_eval_pcd_grouped_workspace_bytes(300, 257), lambda ws: E.eval_pcd_objects(gt, gt_obj, rec, rec_obj, (0.03,), workspace_buffer=ws))
