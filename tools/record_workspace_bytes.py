"""The size of every caller-owned buffer of libdqoraster.so over a fixed argument grid: every *_workspace_bytes export and the
rasteriser context's size queries.  A workspace's size is its layout function at a null base, so a part that moves, grows
or is taken in another order shows here as a changed number.  tests/workspace_bytes_parent.json holds the table of the commit before
the layouts were unified; tests/test_workspace_layouts.py rebuilds it from the library of the tree and compares entry by entry.

The grid sits on the steps where a part crosses a 256-byte alignment or a span of 2048: mesh capacities, the sampler's face counts,
TSDF dims, image sizes (MS-SSIM's and LPIPS' smallest sides among them), point counts — and arguments every query must answer with 0.

A size query added after that commit has no parent to be held to.  It goes on a second grid (_queries_since) with a table of its own,
tests/workspace_bytes_since.json, recorded from the commit that adds it and held by that commit's own test
(tests/test_mesh_render_abi.py); exports() names the declared queries that are NOT on the second grid, exports_since() those that are —
so a declared query that is on no grid still fails the first test.  The exact point-to-triangle distance's two queries are a third grid
of the same kind (_queries_surface, tests/workspace_bytes_surface.json, held by tests/test_mesh_dist_abi.py).

    python tools/record_workspace_bytes.py [--lib path/to/libdqoraster.so] [--out tests/workspace_bytes_parent.json]
    python tools/record_workspace_bytes.py --since [--out tests/workspace_bytes_since.json]
    python tools/record_workspace_bytes.py --surface [--out tests/workspace_bytes_surface.json]
"""
import argparse
import ctypes
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dqo-map_amd"))
from _dqo_native import PROTOTYPES  # noqa: E402

DEFAULT_LIB = os.path.join(ROOT, "dqo-map_amd", "lib", "libdqoraster.so")
DEFAULT_OUT = os.path.join(ROOT, "tests", "workspace_bytes_parent.json")

MESH_CAPS = [1, 2, 255, 256, 257, 2047, 2048, 2049, 6498, 100000, 1 << 22, (1 << 28) - 1]
MESH_BAD = [(0, 1), (1, 0), (-1, 5), (1 << 28, 1), (1, 1 << 28)]
SAMPLE_F = [1, 1023, 1024, 1025, 100000, (1 << 25) - 1]
SAMPLE_COUNT = [1, 257, (1 << 25) - 1]
SAMPLE_BAD = [(0, 1), (1, 0), (1 << 25, 1), (1, 1 << 25)]
TSDF_DIMS = [(2, 2, 2), (3, 5, 7), (65, 4, 3), (64, 64, 64), (645, 645, 645)]
TSDF_BAD = [(1, 2, 2), (2, 2, 0), (646, 646, 646), (1 << 28, 2, 2)]
IMAGES = [(1, 1), (15, 17), (16, 16), (33, 17), (64, 48), (1200, 680)]
IMAGES_LPIPS = [(31, 31), (31, 47), (64, 48)]      # both sides at least 31
IMAGES_MSSSIM = [(161, 161), (161, 203), (203, 177)]  # both sides above 160
IMAGES_BAD = [(0, 1), (1, 0), (-3, 5), (46341, 46341)]
POINTS = [1, 255, 256, 4097, (1 << 25) - 1]
POINTS_BAD = [-1, 1 << 25]

def _queries():
    """(export, argument tuples)"""
    mesh = list(itertools.product(MESH_CAPS, MESH_CAPS)) + MESH_BAD
    for name in ("components", "smooth", "normals", "simplify", "cull"):
        yield f"dqo_mesh_{name}_workspace_bytes", mesh
    sample = list(itertools.product(SAMPLE_F, SAMPLE_COUNT)) + SAMPLE_BAD
    yield "dqo_mesh_sample_workspace_bytes", sample
    yield "dqo_mesh_sample_counted_workspace_bytes", sample
    yield "dqo_tsdf_workspace_bytes", TSDF_DIMS + TSDF_BAD
    images = IMAGES + IMAGES_LPIPS + IMAGES_MSSSIM + IMAGES_BAD
    for name in ("dqo_map_ssim_workspace_bytes", "dqo_growth_sample_workspace_bytes", "dqo_eval_picture_workspace_bytes",
                 "dqo_window_masks_workspace_bytes", "dqo_eval_ms_ssim_workspace_bytes", "dqo_eval_lpips_workspace_bytes",
                 "dqo_track_preprocess_workspace_bytes"):
        yield name, images
    yield "dqo_rast_image_bytes", IMAGES + IMAGES_LPIPS + IMAGES_MSSSIM  # (no argument check of its own)
    points = POINTS + POINTS_BAD
    for name in ("dqo_knn3_workspace_bytes", "dqo_prune_workspace_bytes", "dqo_map_lifecycle_workspace_bytes", "dqo_map_pack_workspace_bytes",
                 "dqo_map_attach_workspace_bytes", "dqo_eval_ate_workspace_bytes"):
        yield name, [(n,) for n in [0] + points]
    pairs = list(itertools.product([0] + POINTS, [0] + POINTS)) + [(-1, 1), (1, 1 << 25)]
    for name in ("dqo_knn3_query_workspace_bytes", "dqo_nn1_workspace_bytes", "dqo_nn1_grouped_workspace_bytes", "dqo_eval_pcd_workspace_bytes",
                 "dqo_eval_pcd_grouped_workspace_bytes"):
        yield name, pairs
    yield "dqo_rast_geom_bytes", [(n, 1200, 680) for n in [0] + points]
    caps = [0, 1, 255, 256, 4097, 1 << 22, -1]
    yield "dqo_rast_binning_bytes", [(c,) for c in caps]
    yield "dqo_rast_backward_workspace_bytes", [(c,) for c in caps]
    yield "dqo_rast_binning_bytes_bucketed", [(c, w, h, b) for c in (0, 4097) for w, h in IMAGES for b in (0, 64, 1000)]
    yield "dqo_surfel_densify_workspace_bytes", [(n, c, l, s) for n in [0] + points for c, l, s in ((8, 1, 1), (12, 3, 2), (0, 1, 1))]
    for name in ("dqo_icp_workspace_bytes", "dqo_map_loss_workspace_bytes", "dqo_track_pyramid_workspace_bytes", "dqo_track_p2p_workspace_bytes"):
        yield name, [()]


STACKS = [(n, w, h) for n in (1, 2, 33, 100) for w, h in IMAGES]  # (n_views, W, H)
STACKS_BAD = [(0, 8, 8), (65536, 8, 8), (1, 0, 8), (1, 8, -1), (1, 1 << 24, 1 << 24)]


def _queries_since():
    """the size queries added since the parent table was recorded: (export, argument tuples)"""
    yield "dqo_mesh_render_depth_workspace_bytes", STACKS + STACKS_BAD
    yield "dqo_eval_depth_l1_workspace_bytes", STACKS + STACKS_BAD


SURFACE_SIZES = [1, 63, 64, 65, 1023, 1025, 4097, 70001, (1 << 25) - 1]
SURFACE_BAD = [(0, 8, 8), (8, 0, 8), (8, 8, 0), (-1, 8, 8), (1 << 25, 8, 8), (8, 1 << 28, 8), (8, 8, 1 << 25)]
SURFACE_SIDES = [(0, 0, 0), (1, 0, 0), (4097, 0, 0), (4097, 300, 1025), (70001, 40000, 70001), ((1 << 25) - 1, (1 << 28) - 1, (1 << 25) - 1)]
SURFACE_SIDES_BAD = [(-1, 0, 0), (1 << 25, 0, 0), (8, 0, 5), (8, 5, 0), (8, 5, 1 << 25), (8, 1 << 28, 5)]  # (points, cap_vertices, cap_faces)


def _queries_surface():
    """the third grid: dqo_mesh_nearest's and dqo_eval_pcd_surface's size queries: (export, argument tuples)"""
    yield "dqo_mesh_nearest_workspace_bytes", [(q, 1000, f) for q in SURFACE_SIZES for f in SURFACE_SIZES] + SURFACE_BAD
    sides = [g + r for g in SURFACE_SIDES for r in SURFACE_SIDES]
    yield "dqo_eval_pcd_surface_workspace_bytes", sides + [b + SURFACE_SIDES[1] for b in SURFACE_SIDES_BAD] + [SURFACE_SIDES[1] + b for b in SURFACE_SIDES_BAD]


def key(name, args):
    return f"{name}({', '.join(str(a) for a in args)})"


def table(lib_path=DEFAULT_LIB, queries=_queries):
    """{"export(arguments)": bytes} over the grid, from the library at lib_path"""
    lib = ctypes.CDLL(lib_path)
    out = {}
    for name, rows in queries():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = PROTOTYPES[name]  # (the binding's, read from the header)
        for args in rows:
            out[key(name, args)] = int(fn(*args))
    return out


def table_since(lib_path=DEFAULT_LIB):
    """the second grid's table (tests/workspace_bytes_since.json)"""
    return table(lib_path, _queries_since)


def table_surface(lib_path=DEFAULT_LIB):
    """the third grid's table (tests/workspace_bytes_surface.json)"""
    return table(lib_path, _queries_surface)


def _declared(header_path):
    import re
    return set(re.findall(r"^size_t (dqo_\w+_bytes\w*)\(", open(header_path).read(), re.M))


def exports(header_path=os.path.join(ROOT, "include", "dqo_raster.h")):
    """the size queries the public header declares, less those of the later grids: the first grid must name every one of them"""
    return sorted(_declared(header_path) - {name for name, _ in _queries_since()} - {name for name, _ in _queries_surface()})


def exports_since(header_path=os.path.join(ROOT, "include", "dqo_raster.h")):
    """the size queries of the second grid that the public header declares"""
    return sorted(_declared(header_path) & {name for name, _ in _queries_since()})


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--lib", default=DEFAULT_LIB)
    ap.add_argument("--out", default=None)
    ap.add_argument("--since", action="store_true", help="the second grid: the queries added since the parent table was recorded")
    ap.add_argument("--surface", action="store_true", help="the third grid: the exact point-to-triangle distance's size queries")
    a = ap.parse_args()
    t = table_surface(a.lib) if a.surface else table_since(a.lib) if a.since else table(a.lib)
    a.out = a.out or (os.path.join(ROOT, "tests", "workspace_bytes_surface.json" if a.surface else "workspace_bytes_since.json")
                      if a.surface or a.since else DEFAULT_OUT)
    with open(a.out, "w") as f:
        json.dump(t, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(t)} entries -> {a.out}")
