"""CPU-side checks of the tracker's C-ABI entry points (dqo_icp_gauss_newton, dqo_track_*): size queries, and argument validation
that happens before any launch (-1 for bad arguments, -2 for a short workspace; usable without a GPU), plus the Python surface."""
import ctypes
import inspect

import pytest


@pytest.fixture(scope="module")
def native():
    import __graft_entry__ as g
    g.build_hip()
    import _dqo_native
    return _dqo_native


def test_size_queries(native):
    lib = native.lib()
    assert lib.dqo_track_pyramid_pixels(680, 1200, 3) == 170 * 300 + 340 * 600 + 680 * 1200
    assert lib.dqo_track_pyramid_pixels(50, 70, 3) == 12 * 17 + 25 * 35 + 50 * 70  # floor sizes, as MaxPool2d
    assert lib.dqo_track_pyramid_pixels(680, 1200, 5) == -1 and lib.dqo_track_pyramid_pixels(0, 10, 1) == -1
    assert lib.dqo_track_preprocess_workspace_bytes(680, 1200) >= 16 * 680 * 1200
    assert lib.dqo_track_preprocess_workspace_bytes(-1, 10) == 0
    assert lib.dqo_track_pyramid_workspace_bytes() > 0 and lib.dqo_track_p2p_workspace_bytes() > 0


def test_argument_validation_before_launch(native):
    lib = native.lib()
    p = 1  # any non-NULL address: validation fails before anything is dereferenced or launched
    big = 1 << 30
    assert lib.dqo_icp_gauss_newton(1, 10, p, p, p, p, p, p, 1.0, 0.1, 0.9, 1e-4, p, p, big, None) == -1
    assert lib.dqo_icp_gauss_newton(10, 10, p, None, p, p, p, p, 1.0, 0.1, 0.9, 1e-4, p, p, big, None) == -1
    assert lib.dqo_icp_gauss_newton(10, 10, p, p, p, p, p, None, 1.0, 0.1, 0.9, 1e-4, p, p, big, None) == -1  # no intrinsics
    assert lib.dqo_icp_gauss_newton(10, 10, p, p, p, p, p, p, 1.0, 0.1, 0.9, 1e-4, p, p, 8, None) == -2
    assert b"workspace" in lib.dqo_last_error()

    assert lib.dqo_track_preprocess(0, 10, p, p, 0.3, 5, 0.2, 0, p, p, p, p, p, p, big, None) == -1
    assert lib.dqo_track_preprocess(10, 10, p, p, 0.3, 5, 0.2, 0, p, p, None, p, p, p, big, None) == -1
    assert lib.dqo_track_preprocess(10, 10, p, None, 0.3, 5, 0.2, 0, p, p, p, p, p, p, big, None) == -1
    assert lib.dqo_track_preprocess(10, 10, p, p, 0.3, 5, 0.2, 0, p, p, p, p, p, p, 16, None) == -2

    assert lib.dqo_track_pyramid(16, 16, 0, p, p, p, p, p, big, None) == -1
    assert lib.dqo_track_pyramid(16, 16, 5, p, p, p, p, p, big, None) == -1
    assert lib.dqo_track_pyramid(3, 16, 3, p, p, p, p, p, big, None) == -1  # level 0 would be 0 rows
    assert lib.dqo_track_pyramid(16, 16, 3, p, p, None, p, p, big, None) == -1
    assert lib.dqo_track_pyramid(16, 16, 3, p, None, p, p, p, big, None) == -1
    assert lib.dqo_track_pyramid(16, 16, 3, p, p, p, p, None, big, None) == -2

    assert lib.dqo_track_fill_model_depth(-4, 10, p, p, p, p, 0.01, 0.01, None) == -1
    assert lib.dqo_track_fill_model_depth(4, 10, p, p, None, p, 0.01, 0.01, None) == -1

    assert lib.dqo_track_p2p_loss(0, 10, p, p, p, p, 0.02, p, p, p, p, p, big, None) == -1
    assert lib.dqo_track_p2p_loss(10, 10, p, p, p, p, 0.02, p, p, p, None, p, big, None) == -1  # count without ratio
    assert lib.dqo_track_p2p_loss(10, 10, p, p, p, p, 0.02, None, p, None, None, p, big, None) == -1  # no success
    assert lib.dqo_track_p2p_loss(10, 10, p, p, p, p, 0.02, None, p, p, None, p, 4, None) == -2


def test_python_surface_matches_reference(native):
    import dqo_icp
    assert list(inspect.signature(dqo_icp.preprocess_frame).parameters) == [
        "depth", "K", "min_depth", "max_depth", "invalid_confidence_thresh", "depth_filter"]
    T = dqo_icp.IcpTracker
    assert list(inspect.signature(T.update_curr_status).parameters) == ["self", "depth_t1", "K"]
    assert list(inspect.signature(T.move_last_status).parameters) == ["self"]
    assert list(inspect.signature(T.update_last_status).parameters) == ["self", "frame", "render_depth", "frame_depth", "render_normal",
                                                                        "frame_normal"]
    assert list(inspect.signature(T.predict_pose).parameters) == ["self", "frame"]
    assert list(inspect.signature(T.predict_pose_async).parameters) == ["self", "frame"]
