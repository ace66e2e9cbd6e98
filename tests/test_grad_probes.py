"""CPU pins of the premises of the row-own gradient check (util_rast.compare_grads_own_row, tests/test_gpu_grad_rows.py): each probe
is what it claims — no checked element of the wrong sign, the fp32 oracle passes the bar against fp64, and the disjoint selection
gives every Gaussian at most one pixel's term."""
import numpy as np
import pytest

from dqo_harness import scenes
import util_rast as U


@pytest.fixture(scope="module")
def cfg1():
    return scenes.make_config(1)


def _pair(oracle, cam, sc, **kw):
    o, r, _ = U.run_oracle(oracle, cam, sc, **kw)
    o64, r64, _ = U.run_oracle(oracle, cam, sc, dtype=np.float64, **kw)
    return o, r, o64, U.flipped_pixels(r, r, r64)


def _masked(dL, bad):
    keep = (~bad).astype(np.float32)
    return dL[0] * keep[None], dL[1] * keep[None]


@pytest.mark.parametrize("bg", [(0, 0, 0), (0.3, 0.5, 0.7)])
def test_colour_probe_has_no_negative_colour_term(oracle, cfg1, bg):
    """dL/dcolor >= 0, dL/ddepth = 0: the colour gradient is sum(alpha T dL) >= 0, and each SH coefficient's gradient has the sign of
    its basis function at the Gaussian's view direction (the same sign on all three channels' non-zero entries of a coefficient)."""
    cam, sc = cfg1
    o, r, o64, bad = _pair(oracle, cam, sc, bg=bg)
    dL = _masked(U.colour_probe(cam, 1), bad)
    assert (dL[0] >= 0).all() and not dL[1].any()
    g = o64.backward(*dL)
    assert (g.colors >= 0).all()
    # sh[:, k, ch] = basis_k x dL/dcolor[:, ch] (0 where the channel is clamped): per (row, k) no two channels of opposite sign
    assert not ((g.sh > 0).any(2) & (g.sh < 0).any(2)).any()
    st = U.compare_grads_own_row(U.oracle_backward(o, dL), U.oracle_backward(o, dL), U.oracle_backward(o64, dL), keys=("sh",),
                                 rtol=U.OWN_ROW_RTOL / 2)
    assert st["sh"]["nonzero"] > 0.95 * len(sc["xyz"]) and st["sh"]["worst_oracle"] <= U.OWN_ROW_RTOL / 2


def test_uniform_colour_probe_has_no_negative_colour_or_opacity_term(oracle, cfg1):
    cam, sc = cfg1
    cp, dL = U.uniform_colour_probe(cam, len(sc["xyz"]), 2)
    o, r, o64, bad = _pair(oracle, cam, sc, colors_precomp=cp, bg=(0, 0, 0))
    dL = _masked(dL, bad)
    g = o64.backward(*dL)
    assert (g.colors >= 0).all() and (g.opacity >= 0).all()
    og32, og64 = U.oracle_backward(o, dL, True), U.oracle_backward(o64, dL, True)
    st = U.compare_grads_own_row(og32, og32, og64, keys=("colors", "opacity"), rtol=U.OWN_ROW_RTOL / 2)
    for k in ("colors", "opacity"):
        assert st[k]["nonzero"] > 0.95 * len(sc["xyz"]) and st[k]["worst_oracle"] <= U.OWN_ROW_RTOL / 2, (k, st[k])


def test_disjoint_probe_fp32_oracle_passes_the_own_row_bar(oracle, cfg1):
    """All five tensors under the disjoint probe: the fp32 oracle passes compare_grads_own_row against fp64 (its own probe check at
    rtol / 2 inside), and the probe reaches a tenth of the visible rows in eight rounds."""
    cam, sc = cfg1
    o, r, o64, bad = _pair(oracle, cam, sc)
    vis = r["radii"] > 0
    got = np.zeros_like(vis)
    for p in U.disjoint_pixel_probe(o, r["hit_depth"], 2, 8, exclude=bad):
        assert not (p["pixels"] & bad).any()
        og32, og64 = U.oracle_backward(o, p["dL"]), U.oracle_backward(o64, p["dL"])
        U.compare_grads_own_row(og32, og32, og64, keys=("means3D", "sh", "opacity", "scales", "rotations"))
        for k, v in og64.items():
            nz = (np.abs(v).reshape(len(vis), -1) > 0).any(1)
            assert not (nz & ~p["covered"]).any(), k
            got |= nz
    assert got[vis].mean() >= 0.1, got[vis].mean()


def test_disjoint_selection_gives_one_term_per_gaussian(oracle, cfg1):
    """The backward is linear in the incoming gradient: the sum of single-pixel backwards over chosen pixels equals their combined
    backward.  With a disjoint selection no row is non-zero in two single-pixel backwards, and each pixel's rows lie inside the set
    disjoint_pixels claims for it: every Gaussian's gradient is ONE pixel's term (fp64, 1e-12 of the row)."""
    cam, sc = cfg1
    o64, r64, _ = U.run_oracle(oracle, cam, sc, dtype=np.float64)
    p = U.disjoint_pixel_probe(o64, r64["hit_depth"], 5, 1)[0]
    ys, xs = np.nonzero(p["pixels"])
    assert len(ys) >= 8
    ys, xs = ys[:8], xs[:8]
    dC, dD = np.zeros_like(p["dL"][0]), np.zeros_like(p["dL"][1])
    dC[:, ys, xs], dD[:, ys, xs] = p["dL"][0][:, ys, xs], p["dL"][1][:, ys, xs]
    whole = U.oracle_backward(o64, (dC, dD))
    total = {k: np.zeros(v.shape, np.float64) for k, v in whole.items()}
    owner = np.full(len(sc["xyz"]), -1)
    for j, (y, x) in enumerate(zip(ys, xs)):
        c1, d1 = np.zeros_like(dC), np.zeros_like(dD)
        c1[:, y, x], d1[:, y, x] = dC[:, y, x], dD[:, y, x]
        one = U.oracle_backward(o64, (c1, d1))
        nz = np.zeros(len(owner), bool)
        for k, v in one.items():
            total[k] += v
            nz |= (np.abs(v).reshape(len(owner), -1) > 0).any(1)
        assert (owner[nz] == -1).all(), f"pixel {(y, x)} shares a Gaussian with pixel {owner[nz][owner[nz] >= 0][:1]}"
        assert nz.any() and p["covered"][nz].all()
        owner[nz] = j
    for k in whole:
        e, mag = U.own_row_err(total[k], whole[k])
        assert (e <= 1e-12).all(), (k, float(e.max()))
