"""_dqo_context: the bucket rule, the capacity rule and the header's field names, and the op's bounded hint maps.  No GPU, no library."""
import pytest

import _dqo_context as C
import _dqo_native as N


def _parent_bucket(longest, margin):
    """The rule as _bucket_for and FusedMapper._size_graph each spelled it before there was one bucket_for."""
    b = 256
    while b < 2 * longest:
        b *= 2
    if b == 2048 and margin * longest <= 1024:
        b = 1024
    return b


@pytest.mark.parametrize("margin", [1.3, 2.0])
def test_bucket_for_is_the_parents_rule(margin):
    for n in range(0, 5001):
        assert C.bucket_for(n, margin) == _parent_bucket(n, margin), n
    assert C.bucket_for(300) == C.bucket_for(300, 1.3)  # (1.3 is the default margin)


@pytest.mark.parametrize("n, b13, b20", [(128, 256, 256), (129, 512, 512), (512, 1024, 1024), (513, 1024, 2048), (787, 1024, 2048),
                                         (788, 2048, 2048), (1024, 2048, 2048), (1025, 4096, 4096)])
def test_bucket_for_at_its_boundaries(n, b13, b20):
    # 2 x 128 = 256 still fits the smallest bucket; 1.3 x 787 = 1023.1 <= 1024 < 1.3 x 788 = 1024.4; 2.0 x 512 = 1024 < 2.0 x 513
    assert (C.bucket_for(n, 1.3), C.bucket_for(n, 2.0)) == (b13, b20)


@pytest.mark.parametrize("n", [0, 1, 580972])
def test_capacity_for_reproduces_the_five_spellings(n):
    assert C.capacity_for(n, 1.0) == n + 4096                    # the first measured forward of a shape in 'lazy' / 'deferred'
    assert C.capacity_for(n, 1.25) == int(n * 1.25) + 4096       # _verify_pending, _pooled_set
    assert C.capacity_for(n, 1.5) == int(1.5 * n) + 4096         # FusedMapper._maintain_render
    assert C.capacity_for(n, 1.15) == int(n * 1.15) + 4096       # FusedMapper._size_graph with capture()'s margins
    assert isinstance(C.capacity_for(n, 1.15), int)


def test_header_dict_names_the_six_public_words():
    want = dict(num_rendered=1, num_tiles=2, overflow=3, max_tile_count=4, num_visible=5, num_candidates=6)
    assert C.header_dict([1, 2, 3, 4, 5, 6, 7, 8]) == want
    assert list(C.header_dict([1, 2, 3, 4, 5, 6, 7, 8])) == list(want)  # (and in the order today's dicts have)
    hdr = N.DqoRastHeader(1, 2, 3, 4, 5, 6, 7, 8)
    assert (hdr.stage, hdr.reserved) == (7, 8)
    assert C.header_dict(hdr) == want
    import torch
    assert C.header_dict(torch.arange(1, 9, dtype=torch.int32)) == want
    assert "stage" not in want and "reserved" not in C.header_dict(hdr)


def test_the_hint_maps_are_bounded_and_only_grow():
    import diff_gaussian_rasterization_depth as dgr
    K = dgr._HINT_KEYS
    assert K == 64
    caps, shapes = {}, {}
    for P in range(K + 3):
        assert dgr._raise_hint(caps, (0, P, 64, 48), 100 + P) == 100 + P
        dgr._raise_hint(shapes, (0, P, 64, 48), [10 * P, P])
    for hints in (caps, shapes):
        assert len(hints) == K and [k[1] for k in hints] == list(range(3, K + 3))  # the three oldest are gone, the rest in write order
    # a key that is written again is the newest one, and the next eviction takes the one behind it
    dgr._raise_hint(caps, (0, 3, 64, 48), 1)
    assert list(caps)[-1] == (0, 3, 64, 48) and len(caps) == K
    dgr._raise_hint(caps, (0, 1000, 64, 48), 7)
    assert (0, 4, 64, 48) not in caps and (0, 3, 64, 48) in caps and len(caps) == K
    # values only grow: an int as max(), the shape hint's pair element by element
    assert caps[(0, 3, 64, 48)] == 103 and dgr._raise_hint(caps, (0, 3, 64, 48), 500) == 500 == caps[(0, 3, 64, 48)]
    key = (0, 10, 64, 48)
    assert dgr._raise_hint(shapes, key, [50, 99]) == [100, 99] and dgr._raise_hint(shapes, key, [200, 5]) == [200, 99] == shapes[key]
    assert isinstance(caps[(0, 3, 64, 48)], int) and isinstance(shapes[key], list)
