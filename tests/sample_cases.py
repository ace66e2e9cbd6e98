"""Frames for the tests of dqo_growth_sample (tests/test_sample_oracle.py on the CPU, tests/test_gpu_sample.py on the GPU): every kind of
pixel the statements of Mapping.temp_points_init tell apart."""
import numpy as np

F = np.float32
# adjacent floats: the components sum to -1.2e-7, the NORMALISED ones to exactly 0 — the row add_empty_points drops (gaussian_pointcloud.py:457)
DROPPED_NORMAL = (F(1.9504636526107788), F(-1.9504637718200684), F(0.0))
# the reference's defaults (configs/base.yaml:32-33, 47-52)
DEFAULTS = dict(uniform_sample_num=50000, add_transmission_thres=0.5, add_depth_thres=0.1, add_color_thres=0.1, transmission_sample_ratio=1.0,
                error_sample_ratio=0.05, init_opacity=0.99, xyz_factor=(1.0, 1.0, 0.1))
# the 50 x 36 frame: the reference's ratios on a frame this small would give k = 0 or k = n
SMALL = dict(DEFAULTS, uniform_sample_num=300, transmission_sample_ratio=2.0, error_sample_ratio=0.3)
# the pixel of make_frame that pins the in-place-mask quirk: T above the threshold, depth > 0, a zero normal and a depth error — the strip
# of the redundant first sample_pixels call takes it out of `trans`, so `sample_mask & ~trans` (mapper.py:1326) counts it
QUIRK_PIXEL = 7


def make_frame(H=36, W=50, seed=0, instance=True, kinds=True):
    """(frame_map, model_map) as dicts of numpy arrays in the reference's [H, W, C] layouts.  kinds: mix in zero normals, normals that
    sum to 0, normals whose normalised components sum to 0, depth 0, instance 0, depth_index -1; T lies on both sides of 0.5."""
    rng = np.random.default_rng(seed)
    n = H * W
    depth = rng.uniform(0.5, 3.0, n).astype(F)
    normal = rng.normal(size=(n, 3)).astype(F)
    normal /= np.linalg.norm(normal, axis=1, keepdims=True).astype(F)
    vertex = rng.uniform(-2, 2, (n, 3)).astype(F)
    color = rng.uniform(0, 1, (n, 3)).astype(F)
    inst = np.zeros((n, 3), F)
    inst[:, 0] = (rng.integers(1, 7, n) / 255.0).astype(F)
    inst[:, 1] = (rng.integers(0, 2, n) * 0.25).astype(F)
    T = rng.uniform(0, 1, n).astype(F)
    render_depth = (depth + rng.normal(0, 0.12, n)).astype(F)
    render_color = (color + rng.normal(0, 0.12, (n, 3))).astype(F)
    depth_index = rng.integers(0, 5000, n).astype(np.int32)
    if kinds:
        kind = rng.integers(0, 40, n)
        depth[kind == 0] = 0
        normal[kind == 1] = 0
        normal[kind == 2] = (1, -1, 0)
        normal[kind == 3] = DROPPED_NORMAL
        inst[kind == 4] = 0
        depth_index[(kind == 5) | (kind == 6)] = -1
        q = QUIRK_PIXEL
        depth[q], normal[q], T[q], render_depth[q], depth_index[q], inst[q, 0] = 1.0, 0, 0.9, 2.0, 3, F(2 / 255.0)
        # one dropped normal in each mask, whatever the draw of `kind` gave
        normal[11], depth[11], T[11], inst[11, 0] = DROPPED_NORMAL, 1.0, 0.95, F(3 / 255.0)
        normal[13], depth[13], T[13], render_depth[13], depth_index[13], inst[13, 0] = DROPPED_NORMAL, 1.0, 0.1, 2.0, 9, F(3 / 255.0)
    frame = dict(depth_map=depth.reshape(H, W, 1), vertex_map_w=vertex.reshape(H, W, 3), normal_map_w=normal.reshape(H, W, 3),
                 color_map=color.reshape(H, W, 3), instance_img=inst.reshape(H, W, 3) if instance else None)
    model = dict(render_transmission=T.reshape(H, W, 1), render_depth=render_depth.reshape(H, W, 1),
                 render_color=render_color.reshape(H, W, 3), render_depth_index=depth_index.reshape(H, W, 1))
    return frame, model


def blank_frame(H, W, on, seed=0):
    """A frame whose first-frame mask is exactly the pixels `on` (depth > 0 there, 0 elsewhere), ordinary normals everywhere."""
    frame, model = make_frame(H, W, seed, instance=False, kinds=False)
    depth = np.zeros(H * W, F)
    depth[np.asarray(on, np.int64)] = 1.5
    frame["depth_map"] = depth.reshape(H, W, 1)
    return frame, model
