// The sampling key of dqo_growth_sample (include/dqo_raster.h): a counter-based hash, a pure function of (seed, draw, pixel).
//
//     fmix32(h):  h ^= h >> 16;  h *= 0x85ebca6b;  h ^= h >> 13;  h *= 0xc2b2ae35;  h ^= h >> 16      (murmur3's 32-bit finaliser)
//
//     s   = fmix32(fmix32(seed_lo ^ 0x9e3779b9) ^ seed_hi)          the seed word      (seed_lo / seed_hi: the halves of the 64-bit seed)
//     b   = fmix32(s + draw)                                        the draw word      (draw 0: first frame, 1: transmission, 2: error)
//     key = fmix32(fmix32(pixel ^ b) ^ s)                           two rounds over the pixel's linear index y * W + x
//     key &= 2^key_bits - 1                                         (key_bits = 32: unchanged)
//
// fmix32 is a bijection of the 32-bit words, so at key_bits = 32 the keys of one draw are pairwise different; with fewer bits they tie,
// and a tie goes to the lower pixel index.  All arithmetic is modulo 2^32.  tests/sample_oracle.py states the same rule in numpy.
//
// The object stage's key (dqo_objmap_frame, dqo_objmap_optimize), a pure function of (seed, draw, frame_id, item):
//
//     b   = fmix32(fmix32(s + draw) + frame_id)                     draw 8: a depth sample's column, 9: its row, 10: an optimise step's view
//     key = fmix32(fmix32(item ^ b) ^ s)                            item = d * 32 + sample for the depth samples (d: the detection's index in
//                                                                   the input, before the filter; sample 0..29), uid * 32 + it for the views
//
// A depth sample's pixel: u = int(b0) + key_u mod (int(b2) - int(b0) + 1), v = int(b1) + key_v mod (int(b3) - int(b1) + 1) (int() truncates
// towards zero, an empty range counts as one value), then clamped to the image.  tests/object_oracle.py states the same rule in Python.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define DQO_SAMPLE_HD __host__ __device__ __forceinline__
#else
#define DQO_SAMPLE_HD inline
#endif

DQO_SAMPLE_HD uint32_t dqo_fmix32(uint32_t h) {
    h ^= h >> 16;
    h *= 0x85ebca6bu;
    h ^= h >> 13;
    h *= 0xc2b2ae35u;
    h ^= h >> 16;
    return h;
}

DQO_SAMPLE_HD uint32_t dqo_sample_seed_word(uint64_t seed) {
    return dqo_fmix32(dqo_fmix32((uint32_t)seed ^ 0x9e3779b9u) ^ (uint32_t)(seed >> 32));
}

DQO_SAMPLE_HD uint32_t dqo_sample_draw_word(uint32_t seed_word, uint32_t draw) { return dqo_fmix32(seed_word + draw); }

DQO_SAMPLE_HD uint32_t dqo_sample_key(uint32_t seed_word, uint32_t draw_word, uint32_t pixel, uint32_t key_mask) {
    return dqo_fmix32(dqo_fmix32(pixel ^ draw_word) ^ seed_word) & key_mask;
}

DQO_SAMPLE_HD uint32_t dqo_object_key(uint32_t seed_word, uint32_t draw, uint32_t frame_id, uint32_t item) {
    const uint32_t b = dqo_fmix32(dqo_sample_draw_word(seed_word, draw) + frame_id);
    return dqo_fmix32(dqo_fmix32(item ^ b) ^ seed_word);
}
