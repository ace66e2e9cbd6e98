"""CPU: the oracle of the exact point-to-triangle distance (tests/mesh_dist_oracle.py) held against itself — that the fixtures reach every
branch of the rule of include/dqo_raster.h, that the float32 rule stays near its float64 twin, that the float64 twin is the distance to
the triangle (an independent sampling check), that the pruned oracle equals the brute force, and the premises of the GPU tests."""
import functools

import numpy as np

import mesh_dist_oracle as M
import pcd_oracle as po

THRES = (0.01, 0.1)  # of the room's tests: 20 000 samples a side lie 2.7 cm apart, so the sampled columns are dense around 3 cm — no threshold there
EPS = 2.0 ** -24
HANDFUL = 8  # pairs of a fixture (of about 800 000) on which the clamp may raise E: a count, not a share


@functools.lru_cache(maxsize=None)
def fixtures():
    """{name: (vertices, faces, queries)}: the four meshes of the GPU tests with their queries."""
    v, f = M.grid_mesh()
    meshes = dict(grid=(v, f), walls=M.with_walls(v, f), slivers=M.with_slivers(v, f), far=M.grid_mesh(offset=1e3))
    return {k: (mv, mf, M.queries(mv, mf, 200)) for k, (mv, mf) in meshes.items()}


@functools.lru_cache(maxsize=None)
def room():
    """The evaluation's room: ((gt vertices, gt faces), (rec vertices, rec faces), gt points, rec points, the oracle's
    rec -> gt mesh result, the oracle's gt -> rec mesh result).  20 000 points a side."""
    gt, rec = M.room_meshes()
    gp, rp = M.sample_mesh(*gt, 20000, 1), M.sample_mesh(*rec, 20000, 2)
    return gt, rec, gp, rp, M.nearest_oracle(rp, gt + (None,)), M.nearest_oracle(gp, rec + (None,))


def _pairs(v, f, q):
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    return q[:, None, :], a[None], b[None], c[None]


def test_every_region_and_the_nan_fallback_occur():
    for name, (v, f, q) in fixtures().items():
        D, E, region, x, fallback = M.tri_dist_f32(*_pairs(v, f, q))
        valid = M.face_validity(v, f)[0]
        counts = np.bincount(region[:, valid].ravel(), minlength=7)
        print(name, "regions", counts.tolist(), "fallbacks", int(fallback[:, valid].sum()))
        assert (counts > 0).all(), (name, counts)  # every region on every fixture
        assert np.isfinite(D[:, valid]).all() and (D[:, valid] >= E[:, valid]).all()
    v, f, q = M.nan_sliver()
    valid, header, _ = M.face_validity(v, f)
    D, E, region, x, fallback = M.tri_dist_f32(*_pairs(v, f, q))
    assert valid.all() and header[:4].tolist() == [1, 1, 0, 0]
    assert fallback.all() and region[0, 0] == 2 and E[0, 0] == np.float32(26) and (x[0, 0] == v[0]).all() and D[0, 0] == E[0, 0]
    # in float64 the same face is an ordinary sliver: the point of edge ac under the query, one metre away
    D64, _, region64, x64, fb64 = M.tri_dist_f64(*_pairs(v, f, q))
    assert not fb64.any() and abs(D64[0, 0] - 1.0) < 1e-12


@functools.lru_cache(maxsize=None)
def clamp_mesh():
    """The grid with clamp_cases' faces behind it (50 runs of grid faces, then the constructed ones) and their queries."""
    v, f, _ = fixtures()["grid"]
    cv, cf, cq = M.clamp_cases()
    return np.concatenate([v, cv]), np.concatenate([f, cf + v.shape[0]]), cq, f.shape[0]


def test_the_clamp_is_active_on_constructed_pairs_and_decides_their_minimum():
    """D = fmax(E, B).  On the four fixtures D == E except on a counted handful of pairs (asserted: at most HANDFUL per fixture, and
    D - E within the rounding bound; observed 0 of 768 000 on grid, 0 on walls, slivers and far): the clamp works where a query lies within a few float32 steps of a face, and clamp_cases constructs such pairs.  There D != E, the face is
    the query's NEAREST face of the whole mesh, so the minimum the kernel must return is D and differs from the minimum of E — a search
    without the clamp, or an oracle without it, gives other bits.  B exceeds E only by E's own rounding error: D - E stays within the
    128 eps M^2 of the next test."""
    for name, (v, f, q) in fixtures().items():
        D, E = M.tri_dist_f32(*_pairs(v, f, q))[:2]
        valid = M.face_validity(v, f)[0]
        raised = (D != E)[:, valid]
        Mf = float(max(np.abs(v).max(), np.abs(q).max()))
        print(name, "pairs with D != E:", int(raised.sum()), "of", raised.size)
        # a counted handful: the clamp needs a query within rounding of a face's box, which 36 of a fixture's 240 queries are (those
        # on vertices, edge midpoints and centroids), each for the few faces around it — never a share of the pairs
        assert (D >= E)[:, valid].all() and raised.sum() <= HANDFUL, (name, int(raised.sum()))
        assert (D - E)[:, valid].max() <= 128 * EPS * Mf * Mf, name
    v, f, q, first = clamp_mesh()
    n = q.shape[0]
    assert n >= 10 and M.face_validity(v, f)[0].all()
    D, E = M.tri_dist_f32(*_pairs(v, f, q))[:2]
    own = np.arange(n)
    assert (D[own, first + own] != E[own, first + own]).all() and (D >= E).all()
    Mx = float(max(np.abs(v).max(), np.abs(q).max()))
    assert (D - E).max() <= 128 * EPS * Mx * Mx
    d2, face, _, _ = M.nearest_oracle(q, (v, f, None))
    won = D[own, face] != E[own, face]  # the winning face is one the clamp raised
    differs = d2.view(np.int32) != E.min(axis=1).view(np.int32)  # ... and the result is not the minimum of E
    print("clamp cases:", n, "won by a clamp-active face:", int(won.sum()), "min D != min E:", int(differs.sum()))
    assert won.sum() >= 10 and differs.sum() >= 10
    brute = M.nearest_oracle(q, (v, f, None), brute=True)[0]
    assert brute.view(np.int32).tobytes() == d2.view(np.int32).tobytes() == D.min(axis=1).view(np.int32).tobytes()


def test_float32_rule_against_its_float64_twin():
    """Regions 0-5 (vertices and edges): |E32 - E64| <= 128 eps M^2 per pair, eps = 2^-24, M the largest coordinate magnitude among the
    query and the three corners.  Where from: every difference of two coordinates is at most 2 M and carries eps 2 M; the closest point
    x is off by at most about 8 eps M (an edge parameter d1 / (d1 - d3) has error 6 eps |ap| / |ab|, times |ab|); E = |p - x|^2 with
    |p - x| <= 2 sqrt(3) M changes by 2 |p - x| |dx| <= 56 eps M^2, and its own three products and two sums add 3 eps 12 M^2: 92 eps
    M^2, rounded up.
    Region 6 (interior): va, vb, vc are differences of products and cancel, so v and w carry kappa eps with
    kappa = 8 (|d1 d4| + |d3 d2| + |d5 d2| + |d1 d6| + |d3 d6| + |d5 d4|) / |va + vb + vc| (three roundings per term and the
    division, doubled), and x moves IN THE FACE'S PLANE by at most kappa eps (|ab| + |ac|).  The exact x is the foot of the
    perpendicular, so an in-plane move t changes E by |t|^2 only; the bound is 128 eps M^2 + (kappa eps (|ab| + |ac|))^2, kappa taken
    from the float64 twin.  Observed maxima of |E32 - E64| over the bound: regions 0-5 0.19, region 6 0.043 (in eps M^2: 24.9 and 5.5)."""
    for name, (v, f, q) in fixtures().items():
        p, a, b, c = (t.astype(np.float64) for t in _pairs(v, f, q))
        E32, region = M.tri_dist_f32(*_pairs(v, f, q))[1:3]
        E64 = M.tri_dist_f64(p, a, b, c)[1]
        valid = M.face_validity(v, f)[0]
        Mx = np.maximum(np.abs(p).max(axis=-1), np.maximum(np.abs(a).max(-1), np.maximum(np.abs(b).max(-1), np.abs(c).max(-1))))
        ab, ac = b - a, c - a
        dot = lambda u, w: (u * w).sum(-1)
        d1, d2, d3, d4, d5, d6 = dot(ab, p - a), dot(ac, p - a), dot(ab, p - b), dot(ac, p - b), dot(ab, p - c), dot(ac, p - c)
        den = (d3 * d6 - d5 * d4) + (d5 * d2 - d1 * d6) + (d1 * d4 - d3 * d2)
        with np.errstate(all="ignore"):
            kappa = 8 * (abs(d1 * d4) + abs(d3 * d2) + abs(d5 * d2) + abs(d1 * d6) + abs(d3 * d6) + abs(d5 * d4)) / abs(den)
        move = kappa * EPS * (np.linalg.norm(ab, axis=-1) + np.linalg.norm(ac, axis=-1))
        bound = 128 * EPS * Mx * Mx + np.where(region == 6, move * move, 0.0)
        err = np.abs(E32.astype(np.float64) - E64)
        edge, inner = (region < 6) & valid[None], (region == 6) & valid[None]
        print(name, "max |E32 - E64| / bound: regions 0-5", (err / bound)[edge].max(), "region 6", (err / bound)[inner].max(),
              "; in eps M^2:", (err / (EPS * Mx * Mx))[edge].max(), (err / (EPS * Mx * Mx))[inner].max())
        assert (err <= bound)[edge].all() and (err <= bound)[inner].all(), name


def test_float64_twin_is_the_distance_to_the_triangle():
    """Independent of the region walk: the smallest distance from the query to a dense barycentric sampling of the winning face (49 steps
    per edge) is never below the exact distance and at most one sampling step (the face's longest edge / 49) above it."""
    n = 49
    i, j = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing="ij")
    sel = (i + j) <= n
    u, w = i[sel] / n, j[sel] / n
    for name, (v, f, q) in fixtures().items():
        d2, face, closest, _ = M.nearest_oracle(q, (v, f, None))
        a, b, c = (v[f[face, k]].astype(np.float64) for k in range(3))
        E64 = M.tri_dist_f64(q, a, b, c)[1]
        samples = a[:, None, :] + u[None, :, None] * (b - a)[:, None, :] + w[None, :, None] * (c - a)[:, None, :]
        smin = np.sqrt(((samples - q.astype(np.float64)[:, None, :]) ** 2).sum(-1).min(axis=1))
        step = np.maximum(np.linalg.norm(b - a, axis=1), np.maximum(np.linalg.norm(c - a, axis=1), np.linalg.norm(c - b, axis=1))) / n
        d = np.sqrt(E64)
        slack = 1e-9 * (1 + np.abs(q).max())
        print(name, "max (samples - exact) / step:", ((smin - d) / step).max())
        assert (d <= smin + slack).all() and (smin <= d + step + slack).all(), name


def test_pruned_oracle_equals_the_brute_force():
    for name, (v, f, q) in fixtures().items():
        counts = np.int32([v.shape[0], f.shape[0] - 7])
        keep = np.arange(q.shape[0]) % 5 != 0
        for kw in (dict(), dict(keeps=keep, xforms=(XFORM, None)), dict(xforms=(None, XFORM))):
            A = M.nearest_oracle(q, (v, f, counts), brute=True, **kw)
            B = M.nearest_oracle(q, (v, f, counts), **kw)
            assert A[0].view(np.int32).tobytes() == B[0].view(np.int32).tobytes() and A[3].tolist() == B[3].tolist(), (name, list(kw))
            found = A[1] >= 0
            assert (found == (B[1] >= 0)).all() and (found == np.asarray(kw.get("keeps", np.ones(q.shape[0], bool)))).all()


XFORM = np.array([[0.8, -0.6, 0.0, 0.25], [0.6, 0.8, 0.0, -0.5], [0.0, 0.0, 1.0, 0.125]], np.float32)


def test_validity_rule_and_header_counts():
    v, f = M.grid_mesh(4)
    V, F = v.shape[0], f.shape[0]
    v = np.concatenate([v, np.float32([[0, 0, 5], [1, 0, 5], [2, 0, 5], [np.nan, 0, 0], [9, 9, 9]])])  # three collinear, a NaN, a spare row
    bad = np.int32([[0, 1, -1], [0, 1, V + 4], [0, 0, 1], [V, V + 1, V + 2], [0, 1, V + 3], [1 << 30, 0, 1]])
    f2 = np.concatenate([f, bad, np.int32([[0, 1, 2]])])  # (the last row lies behind the count)
    counts = np.int32([V + 4, F + 6])  # vertex V + 4 is inside the capacity, outside the count
    valid, header, _ = M.face_validity(v, f2, counts)
    assert valid[:F].all() and not valid[F:].any()
    assert header.tolist() == [F + 6, F, 3, 3, 0, 0, 0, 0]  # bad index: -1, V + 4, 2^30; degenerate: repeated, collinear, NaN
    assert M.mesh_counts(v, f2, np.int32([-5, 1 << 30])) == (0, f2.shape[0])


def test_no_distance_of_the_room_lies_at_a_threshold():
    """The premise of the exact counts of tests/test_gpu_eval_pcd_surface.py, as tests/test_pcd_oracle.py states it for the sampled form."""
    gt, rec, gp, rp, to_gt, to_rec = room()
    for d2 in (to_gt[0], to_rec[0], po.nn1_oracle(rp, gp)[0], po.nn1_oracle(gp, rp)[0]):
        d = np.sqrt(d2.astype(np.float64))
        for th in THRES:
            assert (np.abs(d - th) > 1e-4 * th).all() and 0 < (d < th).sum() < d.size, th


def test_surface_distance_of_a_meshs_own_samples_is_zero_and_the_sampled_form_shows_its_floor():
    """A mesh against itself: its samples lie on it, so the surface distance is rounding (below 1e-6 m here), while the distance to the
    nearest of the OTHER draw's samples is the noise floor 0.5 / sqrt(rho) the sampled metrics carry: 20 000 samples on the room's
    59 m^2 give 0.5 / sqrt(339) = 2.7 cm (observed mean: within 15 % of it)."""
    gt, rec, gp, rp, _, _ = room()
    other = M.sample_mesh(*gt, 20000, 7)
    on = np.sqrt(M.nearest_oracle(gp, gt + (None,))[0].astype(np.float64))
    sampled = np.sqrt(po.nn1_oracle(gp, other)[0].astype(np.float64))
    area = 2 * (4 * 3 + 4 * 2.5 + 3 * 2.5)
    floor = 0.5 / np.sqrt(20000 / area)
    print("surface mean", on.mean(), "max", on.max(), "sampled mean", sampled.mean(), "predicted", floor)
    assert on.max() < 1e-6 and abs(sampled.mean() - floor) < 0.15 * floor
