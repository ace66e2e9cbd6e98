"""CPU-side checks of the drop-in boundary: the C-ABI library loads and exports every symbol include/dqo_raster.h declares
(no compute calls: there is no GPU here), size queries behave, and the Python surface mirrors the reference's."""
import ctypes
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    src = open(os.path.join(ROOT, "include", "dqo_raster.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(dqo_[a-z0-9_]+)\s*\(", src)))


@pytest.fixture(scope="module")
def native():
    import __graft_entry__ as g
    g.build_hip()
    import _dqo_native
    return _dqo_native


def test_exports_every_declared_symbol(native):
    lib = ctypes.CDLL(native.LIB_PATH)
    syms = declared_symbols()
    assert len(syms) >= 16
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in include/dqo_raster.h but not exported"
    assert set(native.EXPORTS) == set(syms)


def test_size_queries_and_errors(native):
    lib = native.lib()
    assert lib.dqo_abi_version() == 5
    g1, g2 = lib.dqo_rast_geom_bytes(1000, 640, 480), lib.dqo_rast_geom_bytes(2000, 640, 480)
    assert 0 < g1 < g2 and g1 % 256 == 0
    assert lib.dqo_rast_image_bytes(1200, 680) >= 12 * 1200 * 680
    assert lib.dqo_rast_binning_bytes(1000) >= 20 * 1000
    assert lib.dqo_rast_backward_workspace_bytes(1000) >= 64 * 1000
    assert lib.dqo_knn3_workspace_bytes(5000) > 5000 * 24
    # argument validation happens before any launch: usable without a GPU
    p = native.DqoRastParams(P=-1, W=10, H=10)
    rc = lib.dqo_rast_forward_prepare(ctypes.byref(p), ctypes.byref(native.DqoRastInputs()), ctypes.byref(native.DqoRastOutputs()),
                                      ctypes.byref(native.DqoRastCtx()), None)
    assert rc == -1 and b"bad sizes" in lib.dqo_last_error()
    assert lib.dqo_knn3(-5, None, None, None, None, 0, None) == -1
    assert lib.dqo_knn3(10, 1, 1, 1, None, 0, None) == -2 and b"workspace" in lib.dqo_last_error()


def test_size_queries_return_size_t(native):
    """By rule, not per export: ctypes' default c_int would cut a size at 2 GiB without a sound."""
    lib = native.lib()
    names = [n for n in native.EXPORTS if "_bytes" in n]  # (every *_bytes, and dqo_rast_binning_bytes_bucketed)
    assert len(names) >= 24 and len([n for n in names if n.endswith("_bytes")]) == len(names) - 1
    for n in names + ["dqo_abi_sizeof"]:
        assert getattr(lib, n).restype is ctypes.c_size_t, n


def test_every_export_with_arguments_has_argtypes(native):
    lib = native.lib()
    no_arguments = {"dqo_abi_version", "dqo_last_error", "dqo_map_loss_workspace_bytes", "dqo_icp_workspace_bytes",
                    "dqo_track_pyramid_workspace_bytes", "dqo_track_p2p_workspace_bytes"}
    for n in native.EXPORTS:
        if n not in no_arguments:
            assert getattr(lib, n).argtypes, n


# The workspace check of every entry point that takes (ws, ws_bytes): (the text in front of " workspace too small", its size query,
# the entry point, the arguments before and behind the pair).  Small valid sizes, 1 for every required pointer: the check fails before
# anything is dereferenced or launched.  The texts are the literals of the entry points as they stood in dqo_capi.hip.
WORKSPACE_CHECKS = [
    ("knn", "dqo_knn3_workspace_bytes", (10,), "dqo_knn3", (10, 1, 1, 1), (None,)),
    ("knn query", "dqo_knn3_query_workspace_bytes", (4, 5), "dqo_knn3_query", (4, 1, 5, 1, 1, 1), (None,)),
    ("loss", "dqo_map_loss_workspace_bytes", (), "dqo_map_loss_fwd_bwd", (8, 8, 1, 1, 1, 1, 1, None, 1.0, 1.0, 0.1, 1, 1, 1), (None,)),
    ("ssim", "dqo_map_ssim_workspace_bytes", (16, 12), "dqo_map_ssim_fwd_bwd", (16, 12, 1, 1, 0.2, 1, None, 0, None), (None,)),
    ("attach-loss", "dqo_map_attach_workspace_bytes", (5,), "dqo_map_attach_loss_fwd_bwd", (5, 1, 1, 1, 1, 1, 1, 1, 2, 1, 1, 1, 1), (None,)),
    ("eval_picture", "dqo_eval_picture_workspace_bytes", (16, 12), "dqo_eval_picture", (16, 12, 1, 1, 1, 1, 1, 0.1, 5.0, None, 1, 0), (None,)),
    ("ms_ssim", "dqo_eval_ms_ssim_workspace_bytes", (161, 162), "dqo_eval_ms_ssim", (161, 162, 1, 1, None, 1, 0), (None,)),
    ("nn1", "dqo_nn1_workspace_bytes", (3, 4), "dqo_nn1", (3, 1, None, 4, 1, None, None, None, 1, None), (None,)),
    ("eval_pcd", "dqo_eval_pcd_workspace_bytes", (3, 4), "dqo_eval_pcd", (3, 1, None, 4, 1, None, None, 0, None, 1, 0), (None,)),
    ("surfel densify", "dqo_surfel_densify_workspace_bytes", (2, 3, 2, 1), "dqo_surfel_densify",
     (2, 1, 1, 1, None, 3, 2, 1, 1, 0, 7, 4, 1, None, None, 1, 1), (None,)),
    ("mesh sample", "dqo_mesh_sample_workspace_bytes", (2, 5), "dqo_mesh_sample", (4, 1, 2, 1, 5, 7, 1, None, 1, 1), (None,)),
    ("map pack", "dqo_map_pack_workspace_bytes", (4,), "dqo_map_pack_rows", (4, 1, 0, 1, 1, 1, 1, 1, None, None, None, 1, 4, 1), (None,)),
    ("icp", "dqo_icp_workspace_bytes", (), "dqo_icp_normal_equations", (4, 6, 1, 1, 1, 1, 1, 1.0, 1.0, 2.0, 3.0, 0.1, 0.9, 1, 1, 1), (None,)),
    ("icp", "dqo_icp_workspace_bytes", (), "dqo_icp_gauss_newton", (4, 6, 1, 1, 1, 1, 1, 1, 1.0, 0.1, 0.9, 1e-6, 1), (None,)),
    ("track preprocess", "dqo_track_preprocess_workspace_bytes", (4, 6), "dqo_track_preprocess",
     (4, 6, 1, 1, 0.1, 5.0, 0.5, 1, 1, 1, 1, 1, 1), (None,)),
    ("track pyramid", "dqo_track_pyramid_workspace_bytes", (), "dqo_track_pyramid", (4, 6, 2, 1, 1, 1, 1), (None,)),
    ("track p2p", "dqo_track_p2p_workspace_bytes", (), "dqo_track_p2p_loss", (4, 6, 1, 1, 1, 1, 0.5, None, 1, 1, None), (None,)),
]


@pytest.mark.parametrize("what,query,sizes,entry,head,tail", WORKSPACE_CHECKS, ids=[c[3] for c in WORKSPACE_CHECKS])
def test_workspace_check(native, what, query, sizes, entry, head, tail):
    lib = native.lib()
    need = getattr(lib, query)(*sizes)
    assert need > 0
    # one byte short, then no workspace at all
    for ws, ws_bytes in ((1, need - 1), (None, need)):
        assert getattr(lib, entry)(*head, ws, ws_bytes, *tail) == -2
        assert lib.dqo_last_error().decode() == f"{what} workspace too small ({ws_bytes} < {need})"


def test_python_surface_matches_reference(native):
    import diff_gaussian_rasterization_depth as m
    assert m.GaussianRasterizationSettings._fields == (
        "image_height", "image_width", "tanfovx", "tanfovy", "bg", "scale_modifier", "viewmatrix", "projmatrix", "sh_degree",
        "campos", "opaque_threshold", "normal_threshold", "depth_threshold", "prefiltered", "debug", "cx", "cy", "color_sigma",
        "T_threshold")
    assert m.GaussianRasterizationSettings._field_defaults == {"color_sigma": 3.0, "T_threshold": 0.0001}
    sig = inspect.signature(m.GaussianRasterizer.forward)
    assert list(sig.parameters) == ["self", "means3D", "opacities", "shs", "colors_precomp", "scales", "rotations", "cov3D_precomp",
                                    "tile_mask", "normal_w"]
    assert list(inspect.signature(m.rasterize_gaussians).parameters) == [
        "means3D", "sh", "colors_precomp", "opacities", "scales", "rotations", "cov3Ds_precomp", "tile_mask", "raster_settings"]
    assert hasattr(m.GaussianRasterizer, "markVisible")
    from simple_knn._C import distCUDA2
    assert callable(distCUDA2)


def test_sync_modes_of_the_operator(native):
    """Host logic only: the four modes are accepted, anything else is refused, and the capacity hint of a shape only grows."""
    import diff_gaussian_rasterization_depth as m
    try:
        for mode in ("lazy", "deferred", "graph", "exact"):
            m.set_sync_mode(mode)
            assert m._sync_mode == mode
        with pytest.raises(ValueError):
            m.set_sync_mode("eager")
        m.set_capacity(1234, 64, 48, 1000, device_index=0)
        m.set_capacity(1234, 64, 48, 500, device_index=0)
        assert m._cap_hint[(0, 1234, 64, 48)] == 1000
    finally:
        m.set_sync_mode("exact")
        m._cap_hint.pop((0, 1234, 64, 48), None)


def test_no_cpu_fallback(native):
    import torch
    from simple_knn._C import distCUDA2
    with pytest.raises(RuntimeError, match="no CPU path"):
        distCUDA2(torch.zeros(10, 3))
    import diff_gaussian_rasterization_depth as m
    rs = m.GaussianRasterizationSettings(48, 64, 1.0, 1.0, torch.zeros(3), 1.0, torch.eye(4), torch.eye(4), 3, torch.zeros(3), 0.6,
                                         0.5, 1.0, False, False, 31.5, 23.5)
    with pytest.raises(RuntimeError, match="no CPU path"):
        m.GaussianRasterizer(rs)(means3D=torch.zeros(4, 3), opacities=torch.ones(4, 1), shs=torch.zeros(4, 16, 3),
                                 scales=torch.ones(4, 3), rotations=torch.ones(4, 4))


def test_product_does_not_import_oracle():
    pkg = os.path.join(ROOT, "dqo-map_amd")
    for dp, _, fs in os.walk(pkg):
        for f in fs:
            if f.endswith((".py", ".hip", ".h")):
                txt = open(os.path.join(dp, f)).read()
                assert "oracle_lib" not in txt and "libdqo_oracle" not in txt, f"{f} references the oracle"
    # the analysis scripts under tools/ run on the product only (diagnostics that need the oracle live under tests/)
    for f in os.listdir(os.path.join(ROOT, "tools")):
        if f.endswith((".py", ".sh")):
            txt = open(os.path.join(ROOT, "tools", f)).read()
            assert "from oracle" not in txt and "import oracle" not in txt and "libdqo_oracle" not in txt, f"tools/{f} references the oracle"
