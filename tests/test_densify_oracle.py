"""CPU-side checks of tests/densify_oracle.py, the float64 restatement dqo_surfel_densify is held to on the GPU: against the recorded
torch float32 statement sequence of the reference (tests/golden/densify_golden.npz, written by tests/golden/make_densify_golden.py), the
column layout, the two frames, the subsample's selection rule, and the premises the GPU tests rely on."""
import os

import numpy as np
import pytest

import densify_oracle as O
from sample_oracle import sample_keys

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "densify_golden.npz")


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


def test_fixture_is_small_and_complete(golden):
    assert os.path.getsize(GOLDEN) < 100 * 1024
    assert golden["xyz"].shape == (24, 3) and golden["scaling_raw"].shape == (24, 3) and golden["rotation_raw"].shape == (24, 4)
    assert [tuple(c) for c in golden["cases"]] == [(1, 30, 5), (2, 3, 2), (3, 7, 1)]
    for j, (sigma, circle_num, levels) in enumerate(golden["cases"]):
        assert golden[f"theta_{j}"].shape == (circle_num,) and golden[f"points_{j}"].shape == (24, sigma * circle_num * levels, 3)
        assert golden[f"points_{j}"].dtype == np.float32 and golden[f"normals_{j}"].shape == (24, 3)


@pytest.mark.parametrize("case", [0, 1, 2])
def test_oracle_matches_the_recorded_reference(golden, case):
    sigma, circle_num, levels = (int(v) for v in golden["cases"][case])
    o = O.densify_oracle(golden["xyz"], golden["scaling_raw"], golden["rotation_raw"], golden[f"theta_{case}"], sigma, circle_num, levels)
    bar = O.coordinate_bar(o, golden["xyz"])
    err = np.abs(golden[f"points_{case}"].astype(np.float64) - o["points"])
    print("largest coordinate error / bar:", (err / bar).max())
    assert (err <= bar).all()
    assert np.abs(golden[f"normals_{case}"].astype(np.float64)[:, None, :] - o["normals"]).max() <= O.NORMAL_BAR


def test_premise_scales_of_non_tie_rows_are_apart(golden):
    raw = golden["scaling_raw"]
    ties = set(int(r) for r in golden["tie_rows"])
    for i in range(raw.shape[0]):
        s = np.sort(raw[i].astype(np.float64))
        if i in ties:
            assert (np.diff(s) == 0).any()
        else:
            assert np.diff(s).min() >= 1e-3, i
    assert (np.diff(np.sort(raw[22])) == 0).sum() == 1 and (np.diff(np.sort(raw[23])) == 0).sum() == 2


def test_tie_order_is_lower_index_first():
    raw = np.array([[-3.0, -4.0, -3.0], [-3.0, -3.0, -4.0], [-4.0, -4.0, -3.0], [-2.0, -2.0, -2.0], [-1.0, -2.0, -3.0]], np.float32)
    assert O.scale_order(raw).tolist() == [[1, 0, 2], [2, 0, 1], [0, 1, 2], [0, 1, 2], [2, 1, 0]]


def test_column_layout():
    sigma, circle_num, levels = 3, 7, 2
    b, l, k = O.column_layout(sigma, circle_num, levels)
    c = np.arange(sigma * circle_num * levels)
    assert (k == c % circle_num).all() and (l == (c % (circle_num * levels)) // circle_num).all() and (b == c // (circle_num * levels)).all()
    a, b_ = O.radii(np.array([2.0]), np.array([5.0]), sigma, circle_num, levels)
    f = np.array([np.float32(0.25), np.float32(0.75)], np.float64)
    for blk in range(sigma):
        for lev in range(levels):
            cols = (blk * levels + lev) * circle_num + np.arange(circle_num)
            assert np.allclose(a[0, cols], 2.0 * sigma * f[lev] + 2.0 * blk, rtol=0, atol=1e-15)
            assert np.allclose(b_[0, cols], 5.0 * sigma * f[lev] + 5.0 * blk, rtol=0, atol=1e-15)
    # one level of float32((l + 0.5) / levels) that is no float64 value of the quotient
    a, _ = O.radii(np.array([1.0]), np.array([1.0]), 1, 1, 5)
    assert a[0, 0] == float(np.float32(0.1)) and a[0, 0] != 0.1


def test_frames_agree_for_identity_and_differ_for_a_rotated_row():
    xyz = np.array([[0.5, -1.0, 2.0], [0.5, -1.0, 2.0]], np.float32)
    raw = np.log(np.array([[0.02, 0.3, 0.1], [0.02, 0.3, 0.1]], np.float32))
    rot = np.array([[1, 0, 0, 0], [0.8, 0.3, -0.4, 0.33]], np.float32)
    theta = np.linspace(0.1, 6.0, 30).astype(np.float32)
    ref = O.densify_oracle(xyz, raw, rot, theta, frame="reference")
    sur = O.densify_oracle(xyz, raw, rot, theta, frame="surfel")
    # identity rotation with the scales ascending along (y, x, z): n = e1, p0 = e0, p1 = e2, so stack(p0, n, p1) is the identity
    # matrix and its rows are its columns — the two frames give the same points
    raw_id = np.log(np.array([[0.1, 0.02, 0.3]], np.float32))
    a = O.densify_oracle(xyz[:1], raw_id, rot[:1], theta, frame="reference")["points"]
    b = O.densify_oracle(xyz[:1], raw_id, rot[:1], theta, frame="surfel")["points"]
    assert np.abs(a - b).max() < 1e-9
    assert np.abs(ref["points"][1] - sur["points"][1]).max() > 1e-2
    # the surfel frame's points lie in the plane, the reference frame's of a rotated row do not
    n = sur["normals"][1, 0]
    assert np.abs((sur["points"][1] - xyz[1].astype(np.float64)) @ n).max() < 1e-12
    assert np.abs((ref["points"][1] - xyz[1].astype(np.float64)) @ n).max() > 1e-2
    assert (ref["normals"] == sur["normals"]).all()


@pytest.mark.parametrize("cap", [1, 17, 399, 400, 401])
def test_select_oracle_is_the_n_smallest_keys_ascending(cap):
    P, M = 40, 10
    idx, header = O.select_oracle(P, M, cap, seed=5)
    n = min(P * M, cap)
    keys = sample_keys(5, 3, np.arange(P * M))
    assert len(np.unique(keys)) == P * M  # fmix32 is a bijection: no ties
    assert idx.shape == (n,) and (np.diff(idx) > 0).all()
    assert np.array_equal(idx, np.sort(np.argsort(keys)[:n]))
    assert header[:5] == [P, P * M, 0, n, M]
    t = header[5] & 0xFFFFFFFF
    assert t == (0xFFFFFFFF if n == P * M else np.sort(keys)[n - 1]) and (keys <= t).sum() == n


def test_select_oracle_with_a_row_mask_and_another_seed():
    P, M = 30, 12
    keep = np.ones(P, np.uint8)
    keep[[0, 7, P - 1]] = 0
    idx, header = O.select_oracle(P, M, 100, seed=1, keep=keep)
    assert header[:5] == [P - 3, (P - 3) * M, 0, 100, M] and keep[idx // M].all()
    other, _ = O.select_oracle(P, M, 100, seed=2, keep=keep)
    assert other.shape == idx.shape and not np.array_equal(other, idx)
    none, header = O.select_oracle(P, M, 100, seed=1, keep=np.zeros(P, np.uint8))
    assert none.shape == (0,) and header == [0, 0, 0, 0, M, -1]
