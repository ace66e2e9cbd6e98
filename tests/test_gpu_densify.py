"""GPU: the densified surfel cloud and its subsample (dqo_eval.densify, FusedMapper.densify / evaluate_geometry_densified —
csrc/map_densify.hip) against tests/densify_oracle.py.  Header, keep, n and index are compared EXACTLY; coordinates against the float64
oracle within a bar that is derived, not measured:

    per coordinate c of a point of row i:   2^-23 * (16 * (a_max + b_max) + |mean_c|)

with a_max, b_max the row's largest radii over its columns.  The float32 roundings on the kernel's way to one coordinate: expf 1 ulp;
the quaternion's normalisation three (sum of squares, sqrt, quotient); an entry of R (magnitude up to 1) four; the column's
normalisation two; the radius three ((axis * sigma) * f_l, + axis * b); the product with the table's cosine one (and the table entry's
own half ulp); the two-term dot two; adding the mean one — under ten ulp of 2^-24 relative on an offset of at most a_max + b_max, one
half ulp on the sum, whose magnitude is at most |mean_c| + a_max + b_max.  16 * 2^-23 = 32 half-ulps on the offset leaves a factor of
three; the reference's torch float32 sequence (which normalises the quaternion twice) stays within 0.3 of the bar on the fixture
(tests/test_densify_oracle.py prints it).  Normals: 2^-23 * 8 (quaternion, entries, normalisation: the same count without the radii).
Every case runs twice and must give the same bits."""
import os

import numpy as np
import pytest

import densify_oracle as O

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "densify_golden.npz")


def _t(a):
    import torch
    return torch.tensor(np.ascontiguousarray(a), device="cuda")


def _rows(seed, P):
    """P random surfels: centres in a 6 m box, log scales at least 0.05 apart in a random axis order, quaternions of any length."""
    rng = np.random.default_rng(seed)
    xyz = ((rng.random((P, 3)) - 0.5) * 6).astype(np.float32)
    base = np.array([-5.5, -3.5, -2.5]) + (rng.random((P, 3)) - 0.5) * 0.8
    raw = np.take_along_axis(base, np.argsort(rng.random((P, 3)), 1), 1).astype(np.float32)
    rot = (rng.normal(size=(P, 4)) * (0.5 + 2 * rng.random((P, 1)))).astype(np.float32)
    assert np.diff(np.sort(raw.astype(np.float64), 1), axis=1).min() >= 1e-3
    return xyz, raw, rot


def _theta(seed, circle_num):
    return (np.random.default_rng(seed).random(circle_num) * 2 * np.pi).astype(np.float32)


def _bits(d, n):
    import torch
    torch.cuda.synchronize()
    out = [d["keep"].cpu().numpy().tobytes(), d["header"].cpu().numpy().tobytes(), d["points"][:n].cpu().numpy().tobytes()]
    for k in ("normals", "index"):
        if d[k] is not None:
            out.append(d[k][:n].cpu().numpy().tobytes())
    return out


def _check(xyz, raw, rot, theta, sigma, circle_num, levels, keep=None, sample_nums=None, seed=0, frame="reference"):
    """Runs dqo_eval.densify twice and holds it to the oracle; returns (first result, n, the chosen virtual points)."""
    import torch
    import dqo_eval
    P, M = xyz.shape[0], sigma * circle_num * levels
    cap = P * M if sample_nums is None else min(P * M, sample_nums)
    idx, header = O.select_oracle(P, M, cap, seed=seed, keep=keep)
    n = header[3]
    args = (_t(xyz), _t(raw), _t(rot))
    kw = dict(sigma=sigma, circle_num=circle_num, levels=levels, theta=torch.tensor(theta), keep=None if keep is None else _t(keep),
              sample_nums=sample_nums, seed=seed, frame=frame, want_index=True)
    d = dqo_eval.densify(*args, **kw)
    first = _bits(d, n)
    assert d["points"].shape == (cap, 3) and d["normals"].shape == (cap, 3) and d["index"].shape == (cap,) and d["keep"].shape == (cap,)
    assert d["points"].dtype == torch.float32 and d["index"].dtype == torch.int64 and d["keep"].dtype == torch.uint8
    assert d["header"].cpu().tolist() == header + [dqo_eval.DENSIFY_FRAMES[frame], 0], (d["header"].cpu().tolist(), header)
    assert d["keep"].cpu().numpy().tolist() == [1] * n + [0] * (cap - n)
    assert np.array_equal(d["index"][:n].cpu().numpy(), idx)
    rows, cols = idx // M, idx % M
    used = np.unique(rows)
    o = O.densify_oracle(xyz[used], raw[used], rot[used], theta, sigma, circle_num, levels, frame)
    at = np.searchsorted(used, rows)
    bar = O.coordinate_bar(o, xyz[used])[at, 0]
    err = np.abs(d["points"][:n].cpu().numpy().astype(np.float64) - o["points"][at, cols])
    nerr = np.abs(d["normals"][:n].cpu().numpy().astype(np.float64) - o["normals"][at, cols])
    if n:
        print(f"P {P} M {M} n {n}: largest coordinate error / bar {(err / bar).max():.3f}, normal error / bar {nerr.max() / O.NORMAL_BAR:.3f}")
    assert (err <= bar).all() and (nerr <= O.NORMAL_BAR).all()
    again = dqo_eval.densify(*args, **kw)
    assert _bits(again, n) == first
    return d, n, idx


@pytest.mark.parametrize("case", [0, 1, 2])
def test_a_the_fixture(case):
    g = np.load(GOLDEN)
    sigma, circle_num, levels = (int(v) for v in g["cases"][case])
    d, n, _ = _check(g["xyz"], g["scaling_raw"], g["rotation_raw"], g[f"theta_{case}"], sigma, circle_num, levels)
    assert n == 24 * sigma * circle_num * levels
    # ... and the recorded float32 sequence of the reference itself: both within the bar of the oracle, so within two bars of each other
    o = O.densify_oracle(g["xyz"], g["scaling_raw"], g["rotation_raw"], g[f"theta_{case}"], sigma, circle_num, levels)
    got = d["points"].cpu().numpy().reshape(24, -1, 3).astype(np.float64)
    assert (np.abs(got - g[f"points_{case}"]) <= 2 * O.coordinate_bar(o, g["xyz"])).all()


def test_b_one_row_past_a_block():
    xyz, raw, rot = _rows(1, 257)
    _, n, _ = _check(xyz, raw, rot, _theta(2, 30), 1, 30, 5)
    assert n == 38550


def test_c_row_mask():
    import torch
    xyz, raw, rot = _rows(3, 257)
    keep = np.ones(257, np.uint8)
    keep[::3] = 0
    keep[[0, 256]] = 0
    kept = int(keep.sum())
    d, n, idx = _check(xyz, raw, rot, _theta(4, 30), 1, 30, 5, keep=keep)
    assert n == kept * 150 and keep[idx // 150].all() and d["header"][0].item() == kept
    # a capacity between N and P * M: the select passes run and reject nothing
    _, n2, idx2 = _check(xyz, raw, rot, _theta(4, 30), 1, 30, 5, keep=keep, sample_nums=257 * 150 - 1)
    assert n2 == n and np.array_equal(idx2, idx)
    for sample_nums in (None, 1000):
        d, n, _ = _check(xyz, raw, rot, _theta(4, 30), 1, 30, 5, keep=np.zeros(257, np.uint8), sample_nums=sample_nums)
        assert n == 0 and not bool(d["keep"].any()) and d["header"].cpu().tolist() == [0, 0, 0, 0, 150, -1, 0, 0]


def test_d_equal_scales_go_to_the_lower_axis():
    xyz, raw, rot = _rows(5, 8)
    raw[0] = [-3.0, -4.0, -3.0]
    raw[1] = [-3.0, -3.0, -4.0]
    raw[2] = [-4.0, -4.0, -3.0]
    raw[3] = [-4.0, -3.0, -4.0]
    raw[4] = [-3.0, -4.0, -4.0]
    raw[5] = [-3.25, -3.25, -3.25]
    assert O.scale_order(raw[:6]).tolist() == [[1, 0, 2], [2, 0, 1], [0, 1, 2], [0, 2, 1], [1, 2, 0], [0, 1, 2]]
    for frame in O.FRAMES:
        _check(xyz, raw, rot, _theta(6, 7), 2, 7, 3, frame=frame)


E_P, E_N = 600, 90000


@pytest.fixture(scope="module")
def unselected():
    import dqo_eval
    xyz, raw, rot = _rows(7, E_P)
    theta = _theta(8, 30)
    d, n, _ = _check(xyz, raw, rot, theta, 1, 30, 5)
    assert n == E_N
    return xyz, raw, rot, theta, d["points"].cpu().numpy(), d["normals"].cpu().numpy()


@pytest.mark.parametrize("sample_nums", [1, 10000, E_N - 1, E_N, E_N + 1])
def test_e_selection(unselected, sample_nums):
    xyz, raw, rot, theta, all_points, all_normals = unselected
    d, n, idx = _check(xyz, raw, rot, theta, 1, 30, 5, sample_nums=sample_nums, seed=9)
    want, _ = O.select_oracle(E_P, 150, sample_nums, seed=9)
    assert n == min(E_N, sample_nums) and np.array_equal(idx, want)
    # bit for bit the point with that v of the unselected run
    assert d["points"][:n].cpu().numpy().tobytes() == all_points[idx].tobytes()
    assert d["normals"][:n].cpu().numpy().tobytes() == all_normals[idx].tobytes()
    if sample_nums == 10000:
        _, n2, other = _check(xyz, raw, rot, theta, 1, 30, 5, sample_nums=sample_nums, seed=10)
        assert n2 == n and not np.array_equal(other, idx)


def test_e_more_chunks_than_blocks():
    """28 000 rows are 4.2 M virtual points, 2 051 chunks of 2 048: the launches are grid-strided from 2 049 chunks on."""
    xyz, raw, rot = _rows(11, 28000)
    keep = np.ones(28000, np.uint8)
    keep[5::7] = 0
    _, n, idx = _check(xyz, raw, rot, _theta(12, 30), 1, 30, 5, keep=keep, sample_nums=5000, seed=2)
    assert n == 5000 and idx.max() >= 2048 * 2048  # (a chosen point lies in a block's second chunk)


def test_f_surfel_frame_lies_in_the_plane():
    """The off-plane distance |(p - mean) . n| is held to the bound the coordinate bar gives a dot product, sum_c bar_c |n_c| (every
    coordinate is within bar_c of a point that lies in the plane) — up to sqrt(3) times one coordinate's bar, not that bar itself."""
    xyz, raw, rot = _rows(13, 300)
    theta = _theta(14, 30)
    d, n, idx = _check(xyz, raw, rot, theta, 1, 30, 5, frame="surfel")
    o = O.densify_oracle(xyz, raw, rot, theta, 1, 30, 5, "surfel")
    p = d["points"].cpu().numpy().astype(np.float64).reshape(300, 150, 3)
    nrm = o["normals"]
    off_plane = np.abs(((p - xyz[:, None, :].astype(np.float64)) * nrm).sum(-1))
    bar = (O.coordinate_bar(o, xyz) * np.abs(nrm)).sum(-1)  # every coordinate is within its bar of a point of the plane
    print("largest |(p - mean) . n| / bar:", (off_plane / bar).max())
    assert (off_plane <= bar).all()
    ref = O.densify_oracle(xyz, raw, rot, theta, 1, 30, 5, "reference")
    assert np.abs(((ref["points"] - xyz[:, None, :]) * nrm).sum(-1)).max() > 1e-3  # (the reference's frame does leave the plane)


def test_g_mapper_hook():
    import torch
    import dqo_eval
    from dqo_harness import mapping, scenes
    from dqo_harness.fused_mapping import FusedMapper
    dev = torch.device("cuda")
    cam, sc = scenes.make_config(1, P=2000)
    fm = FusedMapper(sc, mapping.make_settings(cam, dev), dev).reserve(300)
    assert fm.P == 2300
    with pytest.raises(RuntimeError, match="track_lifecycle"):
        fm.densify()
    stable = torch.arange(fm.P, device=dev) % 3 != 0
    fm.track_lifecycle(stable_mask=stable)
    rows = fm.stable_rows()
    n_stable = int(rows.sum().item())
    assert n_stable == int((torch.arange(2000) % 3 != 0).sum()) and not bool(rows[2000:].any())
    rng = np.random.default_rng(21)
    gt = _t((np.asarray(sc["xyz"], np.float32)[::2] + rng.normal(0, 0.01, (1000, 3))).astype(np.float32))
    thres = (0.01, 0.03)
    kw = dict(sample_nums=20000, seed=3)
    got = fm.evaluate_geometry_densified(gt, thres, densify=kw).clone()
    d = fm.densify(want_index=True, **kw)
    want = dqo_eval.eval_pcd(gt, d["points"], thres, rec_keep=d["keep"]).clone()
    plain = fm.evaluate_geometry(gt, thres).clone()
    torch.cuda.synchronize()
    b = lambda t: t.cpu().numpy().view(np.uint32).tobytes()
    print("densified", got[:10].tolist(), "one point per Gaussian", plain[:10].tolist())
    assert b(got) == b(want) and b(got) != b(plain) and np.isfinite(got[:10].cpu().numpy()).all()
    hdr = d["header"].cpu().tolist()
    assert hdr[0] == n_stable and hdr[1] == n_stable * 150 and hdr[3] == 20000 and bool(d["keep"].all())
    assert bool(rows[d["index"] // 150].all())
    # rows="all": every Gaussian of the map, the spare rows still excluded; without sample_nums the capacity is P * M
    a = fm.densify(rows="all", want_index=True, want_normals=False)
    assert a["normals"] is None and a["header"].cpu().tolist()[:5] == [2000, 300000, 0, 300000, 150] and a["points"].shape == (345000, 3)
    assert int(a["keep"].sum().item()) == 300000
    # spare and unstable rows contribute nothing: whatever they hold, the same bits come out
    before = _bits(d, 20000)
    fm.xyz.data[~rows] = 1e3
    fm.scaling_raw.data[~rows] = 2.0
    fm.rotation_raw.data[~rows] = 0.0
    assert _bits(fm.densify(want_index=True, **kw), 20000) == before
    with pytest.raises(RuntimeError, match="sample_nums"):
        fm.evaluate_geometry_densified(gt, thres, densify=dict(sample_nums=1 << 25))
