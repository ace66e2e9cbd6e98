"""The operator's parameter form (rasterize_gaussian_params, dqo_rast_*_params): fed with the map's raw parameters, it must give the
bits of the activated entry fed with dqo_map_activate's outputs and torch.cat([f_dc, f_rest], 1), and gradients that are the activated
entry's chained through the activation Jacobians — in every sync mode, on pooled contexts, with the same number of launches."""
import numpy as np
import pytest

from dqo_harness import scenes
import util_rast as U

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch


def _raw(torch, sc, rest, seed=0):
    """Raw parameters whose activations are the scene's (up to rounding): logit opacity, log scale, a rotation of random length."""
    rng = np.random.default_rng(seed)
    P = sc["xyz"].shape[0]
    t = lambda a: torch.tensor(np.ascontiguousarray(a, np.float32), device="cuda")
    op = np.clip(sc["opacity"].reshape(P, 1).astype(np.float64), 1e-4, 1 - 1e-4)
    shs = sc["shs"]
    f_rest = np.zeros((P, rest, 3), np.float32)
    k = min(rest, shs.shape[1] - 1)
    f_rest[:, :k] = shs[:, 1:1 + k]
    return dict(xyz=t(sc["xyz"]), f_dc=t(shs[:, :1]), f_rest=t(f_rest), opacity_raw=t(np.log(op / (1 - op))),
                scaling_raw=t(np.log(sc["scales"].astype(np.float64))),
                rotation_raw=t(sc["rotations"] * rng.uniform(0.5, 2.0, (P, 1))))


def _activate(torch, r):
    import _dqo_native as N
    P = r["xyz"].shape[0]
    o, s, q = (torch.empty((P, 1), device="cuda"), torch.empty((P, 3), device="cuda"), torch.empty((P, 4), device="cuda"))
    N.check(N.lib().dqo_map_activate(P, N.ptr(r["opacity_raw"]), N.ptr(r["scaling_raw"]), N.ptr(r["rotation_raw"]), N.ptr(o), N.ptr(s),
                                     N.ptr(q), N.current_stream()))
    return o, s, q


def _leaves(r):
    return {k: v.detach().clone().requires_grad_(True) for k, v in r.items()}


def _run_params(torch, rs, r, tm, dL):
    import diff_gaussian_rasterization_depth as dgr
    x = _leaves(r)
    out = dgr.rasterize_gaussian_params(x["xyz"], x["f_dc"], x["f_rest"], x["opacity_raw"], x["scaling_raw"], x["rotation_raw"], tm, rs)
    res = [o.detach().clone() for o in out]
    if dL is None:
        return res, None
    gs = torch.autograd.grad([out[0], out[1]], list(x.values()), list(dL))
    return res, dict(zip(x, gs))


def _run_anchor(torch, rs, r, tm, dL):
    import diff_gaussian_rasterization_depth as dgr
    o, s, q = _activate(torch, r)
    sh = torch.cat([r["f_dc"], r["f_rest"]], 1)
    leaves = dict(xyz=r["xyz"].clone(), sh=sh, opacity=o, scales=s, rotations=q)
    leaves = {k: v.detach().requires_grad_(True) for k, v in leaves.items()}
    e = torch.empty(0, device="cuda")
    out = dgr.rasterize_gaussians(leaves["xyz"], leaves["sh"], e, leaves["opacity"], leaves["scales"], leaves["rotations"], e, tm, rs)
    res = [t.detach().clone() for t in out]
    if dL is None:
        return res, None, (o, s, q)
    gs = torch.autograd.grad([out[0], out[1]], list(leaves.values()), list(dL))
    return res, dict(zip(leaves, gs)), (o, s, q)


def _dL(torch, cam, seed=1):
    rng = np.random.default_rng(seed)
    t = lambda a: torch.tensor(a.astype(np.float32), device="cuda")
    return t(rng.standard_normal((3, cam.H, cam.W))), t(rng.standard_normal((1, cam.H, cam.W)))


def _eq(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, what
    assert torch_equal(a, b), f"{what}: {int((a != b).sum())} elements differ"


def torch_equal(a, b):
    import torch
    return bool(torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b))


def _check_grads(torch, ga, gp, act, r, radii):
    o, s, q = act
    _eq(gp["xyz"], ga["xyz"], "means3D")
    _eq(gp["f_dc"], ga["sh"][:, :1].contiguous(), "f_dc")
    _eq(gp["f_rest"], ga["sh"][:, 1:].contiguous(), "f_rest")
    # the Jacobians of dqo_adam.h, one float32 op at a time
    _eq(gp["opacity_raw"], ga["opacity"] * (o * (1.0 - o)), "opacity_raw")
    _eq(gp["scaling_raw"], ga["scales"] * s, "scaling_raw")
    g, qr = ga["rotations"].double(), r["rotation_raw"].double()
    y, n = q.double(), qr.norm(dim=1, keepdim=True).clamp_min(1e-12)
    want = (g - y * (y * g).sum(1, keepdim=True)) / n
    tol = 4 * 2.0 ** -24 * g.abs().amax(1, keepdim=True) / n
    err = (gp["rotation_raw"].double() - want).abs()
    assert bool((err <= tol).all()), f"rotation_raw: max error / tolerance {float((err / tol.clamp_min(1e-30)).max())}"
    culled = radii == 0  # (the forward's radii output: exactly the culled rows; cfg 1's frustum cloud has none, the room many)
    assert not bool(culled.all())
    for k in ("opacity_raw", "scaling_raw", "rotation_raw", "f_dc", "f_rest"):
        rows = gp[k].reshape(gp[k].shape[0], -1)[culled]
        assert bool((rows == 0).all()), k


CASES = [  # (cfg, P, sh_degree, rest coefficients, tile mask?, bg)
    (1, 4000, 3, 15, False, (0, 0, 0)),
    (1, 4000, 0, 0, False, (0, 0, 0)),
    (1, 4000, 1, 3, True, (0.2, 0.5, 0.9)),
    (1, 4000, 2, 8, False, (0, 0, 0)),
    (1, 4000, 1, 15, True, (0, 0, 0)),
]


@pytest.mark.parametrize("mode", ["exact", "lazy", "deferred"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: f"cfg{c[0]}-D{c[2]}-R{c[3]}-mask{int(c[4])}-bg{int(c[5][0] > 0)}")
def test_forward_and_gradients_are_the_activated_entrys(torch_cuda, mode, case):
    import diff_gaussian_rasterization_depth as dgr
    torch = torch_cuda
    cfg, P, D, rest, masked, bg = case
    cam, sc = scenes.make_config(cfg, P=P)
    r = _raw(torch, sc, rest)
    rs = U.raster_settings_torch(cam, "cuda", sh_degree=D, bg=bg)
    tm = None
    if masked:
        T = ((cam.H + 15) // 16) * ((cam.W + 15) // 16)
        tm = torch.tensor((np.random.default_rng(3).uniform(size=T) < 0.6).astype(np.int32), device="cuda")
    dL = _dL(torch, cam)
    try:
        dgr.set_sync_mode(mode)
        for it in range(3):  # (lazy / deferred: the first call measures, the later ones run on carried capacities and pooled contexts)
            ha, ga, act = _run_anchor(torch, rs, r, tm, dL)
            hp, gp = _run_params(torch, rs, r, tm, dL)
            if mode != "exact":
                dgr.verify_pending()
            for i, (a, b) in enumerate(zip(ha, hp)):
                _eq(b, a, f"output {i} (iteration {it})")
            _check_grads(torch, ga, gp, act, r, hp[8])
    finally:
        dgr.set_sync_mode("exact")


def _room(P=24000, W=640, H=480, fx=400.0):  # (a P of its own: the lazy modes' capacity hints are kept per (P, W, H))
    """The 640 x 480 surfel room of test_gpu_param_sweep.py (cfg 2's seed), with non-zero higher SH coefficients."""
    cam = scenes.replica_camera(W, H, fx, fx, (W - 1) / 2, (H - 1) / 2)
    return cam, scenes.surfel_room(scenes.CONFIGS[2]["seed"], P, n_objects=4, rest_sigma=0.1)


@pytest.mark.parametrize("mode", ["exact", "lazy", "deferred"])
def test_room_640x480(torch_cuda, mode):
    import diff_gaussian_rasterization_depth as dgr
    torch = torch_cuda
    cam, sc = _room()
    r = _raw(torch, sc, 15, seed=5)
    rs = U.raster_settings_torch(cam, "cuda", sh_degree=3)
    dL = _dL(torch, cam, 7)
    try:
        dgr.set_sync_mode(mode)
        for it in range(3):
            ha, ga, act = _run_anchor(torch, rs, r, None, dL)
            hp, gp = _run_params(torch, rs, r, None, dL)
            if mode != "exact":
                dgr.verify_pending()
            for i, (a, b) in enumerate(zip(ha, hp)):
                _eq(b, a, f"output {i} (iteration {it})")
            _check_grads(torch, ga, gp, act, r, hp[8])
    finally:
        dgr.set_sync_mode("exact")


def test_two_backwards_and_two_forwards_give_the_same_bits(torch_cuda):
    import diff_gaussian_rasterization_depth as dgr
    torch = torch_cuda
    cam, sc = scenes.make_config(1, P=4000)
    r = _raw(torch, sc, 15)
    rs = U.raster_settings_torch(cam, "cuda", sh_degree=3)
    dL = _dL(torch, cam)
    x = _leaves(r)
    out = dgr.rasterize_gaussian_params(x["xyz"], x["f_dc"], x["f_rest"], x["opacity_raw"], x["scaling_raw"], x["rotation_raw"], None, rs)
    g1 = torch.autograd.grad([out[0], out[1]], list(x.values()), list(dL), retain_graph=True)
    g2 = torch.autograd.grad([out[0], out[1]], list(x.values()), list(dL))
    for a, b, k in zip(g1, g2, x):
        _eq(a, b, k)
    h1, _ = _run_params(torch, rs, r, None, None)
    h2, _ = _run_params(torch, rs, r, None, None)
    for i, (a, b) in enumerate(zip(h1, h2)):
        _eq(a, b, f"output {i}")


def _kernel_calls(torch, fn):
    import _dqo_native as N
    N.profile_enable(True)
    N.profile_collect(reset=True)
    fn()
    torch.cuda.synchronize()
    prof = N.profile_collect(reset=True)
    N.profile_enable(False)
    return {k: v[1] for k, v in prof.items()}


_LRS = dict(xyz=0.001, f_dc=0.0005, f_rest=0.0005 / 20.0, opacity_raw=0.05, scaling_raw=0.004, rotation_raw=0.001)


def _adam_loop(torch, dgr, rs, r0, dL, n=5):
    """n iterations of the new entry with DqoAdam moving the six raw tensors; before each, the activated entry renders the same
    parameters on the same shape (one pool serves both).  Returns, per iteration, (new entry's outputs, gradients, parameters after
    the step, the activated entry's outputs and gradients)."""
    from dqo_harness import fused_ops
    x = _leaves(r0)
    opt = fused_ops.DqoAdam([dict(params=[x[k]], lr=_LRS[k], name=k) for k in ("xyz", "f_dc", "f_rest", "opacity_raw", "scaling_raw",
                                                                                "rotation_raw")], lr=0.0, eps=1e-15)
    rec = []
    for _ in range(n):
        ha, ga, _ = _run_anchor(torch, rs, {k: v.detach() for k, v in x.items()}, None, dL)
        opt.zero_grad(set_to_none=True)
        out = dgr.rasterize_gaussian_params(x["xyz"], x["f_dc"], x["f_rest"], x["opacity_raw"], x["scaling_raw"], x["rotation_raw"], None,
                                            rs)
        torch.autograd.backward([out[0], out[1]], list(dL))
        opt.step()
        dgr.verify_pending()
        rec.append(([o.detach().clone() for o in out], {k: v.grad.clone() for k, v in x.items()},
                    {k: v.detach().clone() for k, v in x.items()}, ha, ga))
    return rec


def test_dqo_adam_loop_on_pooled_contexts_interleaved_with_the_activated_entry(torch_cuda):
    import diff_gaussian_rasterization_depth as dgr
    torch = torch_cuda
    cam, sc = scenes.make_config(1, P=20000)
    rs = U.raster_settings_torch(cam, "cuda", sh_degree=3)
    dL = _dL(torch, cam)
    r0 = _raw(torch, sc, 15)
    try:
        dgr.set_sync_mode("deferred")
        dgr.set_context_pool(False)
        fresh = _adam_loop(torch, dgr, rs, r0, dL)
        dgr.set_context_pool(True)
        pooled = _adam_loop(torch, dgr, rs, r0, dL)
        key = (torch.cuda.current_device(), torch.cuda.current_stream().cuda_stream, 20000, cam.W, cam.H)
        assert len(dgr._pool[key]) >= 1
    finally:
        dgr.set_sync_mode("exact")
        dgr.set_context_pool(True)
    for it, (a, b) in enumerate(zip(fresh, pooled)):
        for i, (x, y) in enumerate(zip(a[0], b[0])):
            _eq(y, x, f"output {i}, iteration {it}")
        for part, what in ((1, "gradient"), (2, "parameter")):
            for k in a[part]:
                _eq(b[part][k], a[part][k], f"{what} {k}, iteration {it}")
        for i, (x, y) in enumerate(zip(a[3], b[3])):
            _eq(y, x, f"activated entry output {i}, iteration {it}")
        for k in a[4]:
            _eq(b[4][k], a[4][k], f"activated entry gradient {k}, iteration {it}")
    assert not torch.equal(pooled[0][2]["xyz"], pooled[-1][2]["xyz"])  # (the loop moves the map)


def test_launches_per_pair_are_the_activated_entrys_pf_counterparts(torch_cuda):
    import diff_gaussian_rasterization_depth as dgr
    torch = torch_cuda
    cam, sc = scenes.make_config(1, P=20000)
    rs = U.raster_settings_torch(cam, "cuda", sh_degree=3)
    dL = _dL(torch, cam)
    r = _raw(torch, sc, 15)
    try:
        dgr.set_sync_mode("deferred")
        for _ in range(3):  # (steady state: pooled contexts for both entries)
            _run_anchor(torch, rs, r, None, dL), _run_params(torch, rs, r, None, dL)
        dgr.verify_pending()
        ca = _kernel_calls(torch, lambda: _run_anchor(torch, rs, r, None, dL))
        cp = _kernel_calls(torch, lambda: _run_params(torch, rs, r, None, dL))
        dgr.verify_pending()
    finally:
        dgr.set_sync_mode("exact")
    lib_a = {k: v for k, v in ca.items() if k != "activate_kernel"}  # (the anchor's own activation launch)
    assert sum(cp.values()) == sum(lib_a.values()), (ca, cp)
    for k, n in cp.items():
        assert lib_a.get(k.replace("_pf_kernel", "_kernel")) == n, (k, ca, cp)
    assert cp.get("bin_count_pf_kernel") == 1 and cp.get("gaussian_rows_pf_kernel") == 1 and "gaussian_rows_kernel" not in cp
    assert not any(k in cp for k in ("activate_kernel", "zero_words_kernel"))


def test_every_placement_of_the_late_part_gives_the_same_bits(torch_cuda):
    """DQO_K1_WHERE 0 / 1 / 2 (csrc/dqo_k1_late.h: preprocess_kernel<true, true>, tile_sort_wave_kernel<true, true>, tile_sort_kernel<true, true>; 2 is the
    default above 786432 Gaussians): read once per process, so each placement runs in a child process and reports a digest of the
    outputs and gradients of an exact-mode call and of three deferred calls (pooled: bin_count_kernel<true, true>)."""
    import os, subprocess, sys
    code = r'''
import hashlib, os, sys
sys.path[:0] = [os.environ["DQO_TEST_ROOT"], os.environ["DQO_TEST_ROOT"] + "/dqo-map_amd", os.environ["DQO_TEST_ROOT"] + "/tests"]
import torch
from dqo_harness import scenes
import util_rast as U
import diff_gaussian_rasterization_depth as dgr
import test_gpu_param_form as T
cam, sc = scenes.make_config(1, P=7000)
r = T._raw(torch, sc, 15)
rs = U.raster_settings_torch(cam, "cuda", sh_degree=3)
dL = T._dL(torch, cam, 5)
h = hashlib.sha256()
for mode in ("exact", "deferred", "deferred", "deferred"):
    dgr.set_sync_mode(mode)
    out, g = T._run_params(torch, rs, r, None, dL)
    dgr.verify_pending()
    for t in out + [g[k] for k in sorted(g)]:
        h.update(t.cpu().numpy().tobytes())
print("DIGEST", h.hexdigest())
'''
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    digests = []
    for where in ("0", "1", "2"):
        env = dict(os.environ, DQO_K1_WHERE=where, DQO_TEST_ROOT=root)
        out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr[-2000:]
        digests.append([l for l in out.stdout.splitlines() if l.startswith("DIGEST")][-1])
    assert digests[0] == digests[1] == digests[2]


def test_parity_with_the_cpu_oracle(torch_cuda):
    """Independent of the library: the fp32 / fp64 CPU oracle fed with the activated parameters, its gradients chained to the raw ones
    by map_oracle.raw_grads, against the new entry fed with the raw parameters (util_rast's protocol: flipped pixels get no incoming
    gradient on either side; every gradient row beyond the bar must be explained)."""
    from oracle import oracle_lib as ol
    from oracle import map_oracle
    torch = torch_cuda
    cam, sc = scenes.make_config(1, P=2000)
    r = _raw(torch, sc, 15, seed=11)
    o, s, q = _activate(torch, r)
    act = dict(xyz=sc["xyz"], opacity=o.cpu().numpy().reshape(sc["opacity"].shape), scales=s.cpu().numpy(), rotations=q.cpu().numpy(),
               shs=torch.cat([r["f_dc"], r["f_rest"]], 1).cpu().numpy())
    rs = U.raster_settings_torch(cam, "cuda", sh_degree=3)
    rng = np.random.default_rng(0)
    dL = (rng.normal(size=(3, cam.H, cam.W)).astype(np.float32), rng.normal(size=(1, cam.H, cam.W)).astype(np.float32))
    o32, r32, _ = U.run_oracle(ol, cam, act)
    o64, r64, _ = U.run_oracle(ol, cam, act, dtype=np.float64)
    hp, _ = _run_params(torch, rs, r, None, None)
    h = {k: t.cpu().numpy() for k, t in zip(U.HipRun.names, hp)}
    U.compare_forward(h, r32, r64)
    keep = (~U.flipped_pixels(h, r32, r64)).astype(np.float32)
    dLm = (dL[0] * keep[None], dL[1] * keep[None])
    _, gp = _run_params(torch, rs, r, None, tuple(torch.tensor(a, device="cuda") for a in dLm))
    raw = {k: r[k].cpu().numpy() for k in ("opacity_raw", "scaling_raw", "rotation_raw")}

    def chained(og):
        g_op = np.asarray(og["opacity"])
        op, sg, rot = map_oracle.raw_grads(raw["opacity_raw"].reshape(g_op.shape), raw["scaling_raw"], raw["rotation_raw"], g_op,
                                           og["scales"], og["rotations"])
        return dict(means3D=og["means3D"], sh=og["sh"], opacity=op, scales=sg, rotations=rot)

    og32, og64 = chained(U.oracle_backward(o32, dLm)), chained(U.oracle_backward(o64, dLm))
    hg = dict(means3D=gp["xyz"], sh=torch.cat([gp["f_dc"], gp["f_rest"]], 1), opacity=gp["opacity_raw"], scales=gp["scaling_raw"],
              rotations=gp["rotation_raw"])
    hg = {k: v.cpu().numpy().reshape(np.asarray(og32[k]).shape) for k, v in hg.items()}
    U.compare_grads(hg, og32, og64)


def _graph_problem(torch, P=6000):
    from dqo_harness import mapping
    cam, scene = scenes.make_config(1, P=P)
    scene = {k: v for k, v in scene.items() if k != "normals"}
    dev = torch.device("cuda")
    settings = mapping.make_settings(cam, dev)
    rng = np.random.default_rng(3)
    pert = dict(scene)
    pert["xyz"] = (scene["xyz"] + rng.normal(0, 0.004, scene["xyz"].shape)).astype(np.float32)
    pert["shs"] = scene["shs"].copy()
    pert["shs"][:, 0, :] += rng.normal(0, 0.15, (P, 3)).astype(np.float32)
    with torch.no_grad():
        tgt = mapping.render(settings, mapping.GaussianParams(pert, dev).activated())
    mask = torch.tensor(rng.uniform(size=(cam.H, cam.W)) < 0.8, device=dev) & (tgt["depth_index_map"][0] >= 0)
    return scene, settings, tgt["render"].clone(), tgt["depth"].clone(), mask, dev


def _graph_loop(torch, dgr, scene, settings, gt_color, gt_depth, mask, dev, n_iters, graph):
    """forward (new entry) + masked_mapping_loss + backward + DqoAdam(capturable=True): n_iters iterations eagerly, or one warm-up and
    n_iters - 1 replays of a captured graph ('graph' mode through CapturedIteration)."""
    from dqo_harness import mapping, fused_ops
    params = mapping.GaussianParams(scene, dev)
    opt = fused_ops.DqoAdam(params.param_groups(), lr=0.0, eps=1e-15, capturable=True)
    losses = torch.zeros(n_iters, device=dev)
    cell = torch.zeros((), device=dev)

    def iteration():
        r = dgr.rasterize_gaussian_params(params._xyz, params._features_dc, params._features_rest, params._opacity, params._scaling,
                                          params._rotation, None, settings)
        out = {"render": r[0], "depth": r[1], "color_index_map": r[2], "depth_index_map": r[3], "color_hit_weight": r[4],
               "depth_hit_weight": r[5], "T_map": r[6], "n_touched": r[7], "radii": r[8]}
        loss, _ = fused_ops.masked_mapping_loss(out, gt_color, gt_depth, mask)
        loss.backward()
        opt.step()
        cell.copy_(loss.detach())

    dgr.set_sync_mode("lazy")
    if not graph:
        for it in range(n_iters):
            opt.zero_grad(set_to_none=True)
            iteration()
            losses[it] = cell
        dgr.verify_pending()
    else:
        cap = fused_ops.CapturedIteration(iteration, opt, warmup=1)
        losses[0] = cell
        for it in range(1, n_iters):
            cap.replay()
            losses[it] = cell
        hdr = cap.check()
        assert hdr["overflow"] == 0 and hdr["num_rendered"] > 0
    torch.cuda.synchronize()
    return losses, [p.detach().clone() for p in (params._xyz, params._features_dc, params._features_rest, params._opacity,
                                                 params._scaling, params._rotation)]


def test_graph_mode_replays_like_the_eager_loop(torch_cuda):
    import diff_gaussian_rasterization_depth as dgr
    torch = torch_cuda
    prob = _graph_problem(torch)
    try:
        le, pe = _graph_loop(torch, dgr, *prob, 4, graph=False)
        lg, pg = _graph_loop(torch, dgr, *prob, 4, graph=True)  # (one warm-up iteration, then 3 replays)
    finally:
        dgr.set_sync_mode("exact")
    assert float(le[0]) > float(le[-1]) > 0  # the loop trains
    _eq(lg, le, "losses")
    for a, b, k in zip(pg, pe, ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")):
        _eq(a, b, k)


def test_errors_behave_like_the_activated_entry(torch_cuda):
    import diff_gaussian_rasterization_depth as dgr
    torch = torch_cuda
    cam, sc = scenes.make_config(1, P=500)
    rs = U.raster_settings_torch(cam, "cuda", sh_degree=3)
    r = _raw(torch, sc, 15)
    args = lambda d: (d["xyz"], d["f_dc"], d["f_rest"], d["opacity_raw"], d["scaling_raw"], d["rotation_raw"], None, rs)
    with pytest.raises(RuntimeError, match="Float"):
        dgr.rasterize_gaussian_params(*args(dict(r, opacity_raw=r["opacity_raw"].double())))
    with pytest.raises(RuntimeError, match="GPU"):
        dgr.rasterize_gaussian_params(*args(dict(r, scaling_raw=r["scaling_raw"].cpu())))
    with pytest.raises(RuntimeError, match="coefficients"):
        dgr.rasterize_gaussian_params(*args(dict(r, f_rest=r["f_rest"][:, :8].contiguous())))
    z = {k: v[:0] for k, v in r.items()}
    out = dgr.rasterize_gaussian_params(*args(z))
    ref = dgr.rasterize_gaussians(z["xyz"], torch.cat([z["f_dc"], z["f_rest"]], 1), torch.empty(0, device="cuda"), z["opacity_raw"],
                                  z["scaling_raw"], z["rotation_raw"] / 1.0, torch.empty(0, device="cuda"), None, rs)
    for a, b in zip(out, ref):
        _eq(a, b, "P = 0")
