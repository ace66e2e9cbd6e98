"""CPU: where FusedMapper's whole-map operators live (dqo_harness/map_operators.py) and who owns their scratch.  Needs no built library."""
import inspect

MOVED = ("_maintain_render", "maintain_overflowed", "maintain", "MAINTAIN_DEFAULTS", "prune_floaters", "prune_overflowed", "evaluate",
         "evaluate_ms_ssim", "_evaluate", "make_mesh", "densify", "evaluate_geometry", "evaluate_geometry_densified", "evaluate_geometry_mesh",
         "_object_rows", "evaluate_geometry_objects", "evaluate_geometry_objects_mesh", "pack_rows", "save_model", "save_model_objects",
         "_read_checkpoint", "load_model", "_load_tables", "from_model_ply", "SAMPLE_DEFAULTS", "sample_new", "refresh_window")
SCRATCH = ("_lifecycle", "_maintain_ctx", "_prune_ctx", "_eval_tables", "_eval_ws", "_eval_ms_ws", "_mesh_w2c", "_eval_object_rows",
           "_checkpoint", "_window_ratios", "_window_ws", "_window_flags", "_sample_ctx", "sample_header")
STAYED = ("track_lifecycle", "reserve", "grow", "capture", "replay", "run", "_rows", "_row_count_changed")


def test_the_operators_are_map_operators_and_the_core_names_none_of_their_scratch():
    from dqo_harness import fused_mapping as F
    from dqo_harness import map_operators as O
    assert issubclass(F.FusedMapper, O.MapOperators)
    for name in MOVED:
        assert hasattr(F.FusedMapper, name), name
        assert name in vars(O.MapOperators) and name not in vars(F.FusedMapper), name
        attr = inspect.getattr_static(O.MapOperators, name)
        fn = getattr(attr, "__func__", attr)
        if callable(fn):
            assert fn.__module__ == "dqo_harness.map_operators", name
    for name in STAYED:
        assert name in vars(F.FusedMapper) and name not in vars(O.MapOperators), name
    for name in ("_normalised_settings", "_checked_tile_mask", "_RenderContext"):  # both sides use them: one definition
        assert getattr(F, name) is getattr(O, name) and getattr(O, name).__module__ == "dqo_harness.map_operators", name
    assert {"tile_object_sets", "_ROW_BUFFERS", "_FrameGraph"} <= set(vars(F))
    assert inspect.signature(F.FusedMapper._maintain_render).parameters["tile_mask"].default is None
    src = inspect.getsource(F.FusedMapper._row_count_changed)
    for name in SCRATCH:
        assert name not in src, name
    # every scratch attribute is declared by the one method the constructor calls, the per-P ones by the half _row_count_changed calls
    declared = inspect.getsource(O.MapOperators._init_operator_state) + inspect.getsource(O.MapOperators._drop_row_sized_operator_state)
    for name in SCRATCH:
        assert "self." + name in declared, name
    assert "_init_operator_state()" in inspect.getsource(F.FusedMapper.__init__) and "_drop_row_sized_operator_state()" in src
