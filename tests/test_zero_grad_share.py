"""tests/diag_zero_grad_share.py (the count behind DESIGN.md §4.3's list rule) on a small gated scene: its three criteria nest, and the one
the rule rests on — no pixel blends the Gaussian — is exactly the set of in-view rows whose oracle gradient row is zero."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def test_zero_gradient_share_on_a_small_room():
    import diag_zero_grad_share as Z
    from dqo_harness import scenes
    from oracle import oracle_lib as ol
    cam = scenes.replica_camera(320, 192, 160.0, 160.0, 159.5, 95.5)
    sc = scenes.surfel_room(3, 6000, n_objects=8)
    pix_obj = Z.oracle_pix_obj(ol, cam, sc, 10, omp=False)
    assert pix_obj.shape == (192, 320) and pix_obj.max() >= 1 and (pix_obj >= 0).mean() > 0.02
    out, m = Z.zero_grad_rows(ol, cam, sc, pix_obj, omp=False, masks=True)
    assert out["P"] == 6000 and 0 < out["in_view"] < 6000
    free = m["in_view"] & ~m["attach"]
    # no instance => no pair => not counted by n_touched
    assert not (m["has_pair"] & ~m["has_instance"]).any() and not (m["touched"] & ~m["has_pair"]).any()
    assert out["no_instance"] <= out["no_pair"] <= out["n_touched_zero"]
    assert out["no_pair"] == int((free & ~m["has_pair"]).sum()) > 0
    assert abs(out["f_no_pair"] - out["no_pair"] / out["in_view"]) < 1e-4
    assert 0 < out["attach_in_view"] == int((m["in_view"] & m["attach"]).sum())
    # the gradient rows of the same gated forward: zero exactly where nothing blends the Gaussian
    o, r = Z.forward(ol, cam, sc, False, gaussian_object=np.asarray(sc["obj_id"], np.int32), pixel_object=pix_obj)
    rng = np.random.default_rng(0)
    g = o.backward(rng.normal(size=(3, cam.H, cam.W)).astype(np.float32), rng.normal(size=(1, cam.H, cam.W)).astype(np.float32))
    mag = sum(np.abs(np.asarray(a, np.float64)).reshape(6000, -1).sum(1) for a in (g.means3D, g.sh, g.opacity, g.scales, g.rotations))
    assert (mag[~m["has_pair"]] == 0).all()
    assert (mag[m["has_pair"]] > 0).mean() > 0.99
    # n_touched alone would have claimed rows that do get a gradient
    claimed = free & ~m["touched"] & m["has_pair"]
    assert claimed.any() and (mag[claimed] > 0).mean() > 0.99
