"""CPU: the numpy restatement of the tracker's per-frame chain (tests/tracking_oracle.py) against goldens produced by the reference's
own map_preprocess glue, ImagePyramids / build_*_pyramid, IcpTracker.update_last_status and IcpTracker.predict_pose
(tests/golden/make_tracking_golden.py imports /root/reference/SLAM/utils.py and SLAM/icp.py)."""
import os
import types

import numpy as np

import tracking_oracle as to

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tracking_golden.npz"))
CASES = sorted({k.split("_")[0] for k in G.files})
MIN_DEPTH, MAX_DEPTH, CONF_THRESH = 0.3, 5.0, 0.2
SAMPLE_DIST, SAMPLE_NORMAL = 0.01, 0.01
FAIL_THRESH = {"c0": 0.02, "c1": 1.0}
MASK_TOL = 2e-3  # masks: identical except pixels within fp32 rounding of a threshold
MAP_TOL = 1e-5


def args(case, use_model_depth):
    return types.SimpleNamespace(icp_downscales=[0.25, 0.5, 1.0], icp_downscale_iters=[5, 5, 5], icp_damping=1e-4,
                                 icp_distance_threshold=0.1, icp_normal_threshold=20, icp_sample_distance_threshold=SAMPLE_DIST,
                                 icp_sample_normal_threshold=SAMPLE_NORMAL, icp_fail_threshold=FAIL_THRESH[case], icp_warmup_frames=0,
                                 icp_use_model_depth=use_model_depth, verbose=False)


def inputs(c):
    g = lambda k: G[f"{c}_{k}"].astype(np.float32)
    return dict(K=G[f"{c}_K"], depth0=g("depth0_f16"), depth1=g("depth1_f16"), render_depth=g("render_depth_f16"),
                render_normal=g("render_normal_f16"))


def mask_close(a, b):
    return (np.asarray(a) != np.asarray(b)).mean() <= MASK_TOL


def map_close(a, b, tol=MAP_TOL, mismatch=None):
    """|a - b| <= tol everywhere except, when `mismatch` is given, at pixels where a threshold mask flipped."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    a, b = a.reshape(b.shape), b
    d = np.abs(a - b)
    if d.ndim == 3:
        d = d.max(-1)
    d = d.reshape(d.shape[0], d.shape[1])
    if mismatch is not None:
        d = np.where(mismatch, 0, d)
    return float(d.max()) <= tol


def test_preprocess_matches_reference_goldens():
    for c in CASES:
        x = inputs(c)
        for filt in (0, 1):
            o = to.preprocess(x["depth0"], x["K"], MIN_DEPTH, MAX_DEPTH, CONF_THRESH, depth_filter=bool(filt))
            gi = G[f"{c}_pre{filt}_invalid"]
            assert mask_close(o["invalid"], gi), (c, filt)
            flip = o["invalid"] != gi
            assert map_close(o["depth"], G[f"{c}_pre{filt}_depth"], mismatch=flip), (c, filt)
            if filt == 0:
                assert map_close(o["normal"], G[f"{c}_pre0_normal"], mismatch=flip), c
                assert map_close(o["conf"], G[f"{c}_pre0_conf"], mismatch=flip), c
                assert map_close(o["vertex"], G[f"{c}_pyr_vertex2"], mismatch=flip), c


def test_pyramid_matches_reference_goldens():
    for c in CASES:
        x = inputs(c)
        d = G[f"{c}_pre0_depth"]
        for L, (V, N) in enumerate(to.pyramid(d, x["K"], 3)):
            gv = G[f"{c}_pyr_vertex{L}"]
            assert map_close(V if gv.ndim == 3 else V[..., 2], gv), (c, L)
            assert map_close(N, G[f"{c}_pyr_normal{L}"]), (c, L)


def test_fill_matches_reference_goldens():
    for c in CASES:
        x = inputs(c)
        r = to.fill(x["render_depth"], G[f"{c}_pre0_depth"], x["render_normal"], G[f"{c}_pre0_normal"], SAMPLE_DIST, SAMPLE_NORMAL)
        assert mask_close(r != x["render_depth"][..., 0], G[f"{c}_filled_depth"][..., 0] != x["render_depth"][..., 0]), c
        assert mask_close(r, G[f"{c}_filled_depth"][..., 0]), c


def frame_pair(c, use_model_depth):
    """Oracle pyramids of the golden frame pair, as IcpTracker holds them when predict_pose runs on frame 1."""
    x = inputs(c)
    f0 = to.preprocess(x["depth0"], x["K"], MIN_DEPTH, MAX_DEPTH, CONF_THRESH)
    f1 = to.preprocess(x["depth1"], x["K"], MIN_DEPTH, MAX_DEPTH, CONF_THRESH)
    d_t0 = f0["depth"]
    if use_model_depth:
        d_t0 = to.fill(x["render_depth"], f0["depth"], x["render_normal"], f0["normal"], SAMPLE_DIST, SAMPLE_NORMAL)
    return x, f0, f1, to.pyramid(d_t0, x["K"]), to.pyramid(f1["depth"], x["K"])


def test_predict_pose_matches_reference_goldens():
    for c in CASES:
        for m in (0, 1):
            x, _, _, p0, p1 = frame_pair(c, bool(m))
            pose, ok, loss, ratio = to.predict_pose(p0, p1, x["K"], fail_threshold=FAIL_THRESH[c])
            np.testing.assert_allclose(pose, G[f"{c}_m{m}_pose"], rtol=0, atol=2e-4)
            assert ok == bool(G[f"{c}_m{m}_success"])
            assert abs(loss - G[f"{c}_m{m}_loss"]) <= 1e-3 * G[f"{c}_m{m}_loss"] + 1e-6, (c, m, loss)
            assert abs(ratio - G[f"{c}_m{m}_valid_ratio"]) < 5e-3
