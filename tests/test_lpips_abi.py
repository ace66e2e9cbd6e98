"""CPU: dqo_eval_lpips' size queries and its argument checks, every one of which returns before anything touches a device (the pointers
are never followed)."""
import pytest

import lpips_oracle as LO


@pytest.fixture(scope="module")
def native():
    import __graft_entry__ as g
    g.build_hip()
    import _dqo_native
    return _dqo_native


def test_weight_count_is_the_sum_of_the_layer_sizes(native):
    lib = native.lib()
    per_layer = [cin * k * k * cout + 2 * cout for cin, cout, k, _, _ in LO.NET]
    assert [lib.dqo_eval_lpips_weight_floats(l) for l in range(5)] == per_layer
    assert lib.dqo_eval_lpips_weight_floats(-1) == sum(per_layer) == 2470848 == lib.dqo_eval_lpips_weight_floats(5)
    assert sum(cin * k * k * cout for cin, cout, k, _, _ in LO.NET) == 2468544


def test_workspace_bytes(native):
    lib = native.lib()
    assert lib.dqo_eval_lpips_workspace_bytes(30, 31) == 0 and lib.dqo_eval_lpips_workspace_bytes(31, 30) == 0
    assert lib.dqo_eval_lpips_workspace_bytes(-5, 100) == 0 and lib.dqo_eval_lpips_workspace_bytes(40000, 40000) == 0  # (W * H beyond eval_picture's limit)
    n = lib.dqo_eval_lpips_workspace_bytes(31, 31)
    # the ticket words and the means, the five maps of both images (49, 9, 1, 1, 1 pixels), the two pooled maps, 256 lines of partials
    maps = [2 * p * c * 4 for p, c in ((49, 64), (9, 192), (1, 384), (1, 256), (1, 256))] + [2 * 9 * 64 * 4, 2 * 1 * 192 * 4]
    assert n == 4608 + sum((b + 255) // 256 * 256 for b in maps) + 256 * 64 and n % 256 == 0
    assert lib.dqo_eval_lpips_workspace_bytes(1200, 680) > 4 * 2 * 169 * 299 * 64
    import dqo_eval
    import torch
    ws = torch.zeros(n, dtype=torch.uint8)
    for l in range(5):  # the views lie inside the workspace, behind one another
        v = dqo_eval.lpips_feature_view(ws, 31, 31, l)
        assert tuple(v.shape) == (2,) + LO.sizes(31, 31)[l] + (LO.NET[l][1],)
    assert dqo_eval.lpips_feature_view(ws, 31, 31, 0).data_ptr() - ws.data_ptr() == 4608
    assert dqo_eval.lpips_feature_view(ws, 31, 31, 4).data_ptr() - ws.data_ptr() == 4608 + sum((b + 255) // 256 * 256 for b in maps[:4])
    with pytest.raises(RuntimeError, match="31"):
        dqo_eval.lpips_workspace(30, 40, "cpu")


def test_argument_checks_return_before_any_launch(native):
    lib = native.lib()
    n = lib.dqo_eval_lpips_workspace_bytes(67, 45)
    A = 16  # (a non-NULL, 16-byte aligned value for every pointer: none is followed)
    ok = dict(W=67, H=45, image=A, gt=A, weights=A, mode=0, header=None, out=A, row=0, ws=A, ws_bytes=n, stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.dqo_eval_lpips(a["W"], a["H"], a["image"], a["gt"], a["weights"], a["mode"], a["header"], a["out"], a["row"], a["ws"],
                                  a["ws_bytes"], a["stream"])

    for name in ("image", "gt", "weights", "out"):
        assert call(**{name: None}) == -1 and b"null" in lib.dqo_last_error(), name
    assert call(weights=20) == -1 and b"aligned" in lib.dqo_last_error()
    assert call(W=30) == -1 and b"31" in lib.dqo_last_error()
    assert call(H=30) == -1 and b"31" in lib.dqo_last_error()
    assert call(W=40000, H=40000) == -1 and b"size" in lib.dqo_last_error()
    assert call(row=-1) == -1 and b"row" in lib.dqo_last_error()
    for mode in (-1, 2):
        assert call(mode=mode) == -1 and b"norm_mode" in lib.dqo_last_error()
    assert call(ws_bytes=n - 1) == -2 and lib.dqo_last_error().decode() == f"lpips workspace too small ({n - 1} < {n})"
    assert call(ws=None) == -2 and b"workspace" in lib.dqo_last_error()
