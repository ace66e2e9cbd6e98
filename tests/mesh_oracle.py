"""numpy restatement of dqo_mesh_sample (include/dqo_raster.h; csrc/map_meshsample.hip): trimesh.sample.sample_surface's four steps —
face areas, their cumulative sum, one uniform draw located in it, two uniform draws folded back into the triangle — with the seeded key
rule of csrc/dqo_sample_hash.h for the draws and integer quanta of area for the cumulative table.  Imports nothing from the product.

Every float64 statement is written in the order the header gives, one rounding each; the 128-bit product is a Python integer; the face is
np.searchsorted(cum, t, side="right").  trimesh itself does not exist on this platform: this file states the algorithm as its published
source does (sample.py: `area_cum = np.cumsum(area)`, `face_index = np.searchsorted(area_cum, face_pick)`, `random_lengths[random_test]
-= 1.0; random_lengths = np.abs(random_lengths)`, `samples = sample_vector.sum(axis=1) + tri_origins`)."""
import numpy as np

DRAW0 = 4  # draws 4-7 (0-2: the growth sampler's, 3: densify's)
MASK = 0xFFFFFFFF


def fmix32(h):
    h = np.asarray(h, np.uint32).copy()
    with np.errstate(over="ignore"):
        h ^= h >> np.uint32(16)
        h *= np.uint32(0x85EBCA6B)
        h ^= h >> np.uint32(13)
        h *= np.uint32(0xC2B2AE35)
        h ^= h >> np.uint32(16)
    return h


def keys(seed, draw, index):
    """dqo_sample_key(seed_word, dqo_sample_draw_word(seed_word, draw), index, 0xffffffff) for every index: uint32."""
    seed = int(seed) & (2 ** 64 - 1)
    with np.errstate(over="ignore"):
        s = fmix32(fmix32(np.uint32((seed & MASK) ^ 0x9E3779B9)) ^ np.uint32(seed >> 32))
        b = fmix32(s + np.uint32(draw))
        return fmix32(fmix32(np.asarray(index, np.uint32) ^ b) ^ s)


def face_areas(vertices, faces):
    """(A float64 [F], bad bool [F], degenerate bool [F]): a face with an index outside [0, V) has A = 0 (bad) and its vertices are not
    read; a zero or non-finite area among the others becomes 0 (degenerate)."""
    v, f = np.asarray(vertices, np.float32), np.asarray(faces, np.int64).reshape(-1, 3)
    V = v.shape[0]
    bad = ((f < 0) | (f >= V)).any(axis=1)
    g = np.where(bad[:, None], 0, f)
    a, b, c = (v[g[:, k]].astype(np.float64) for k in range(3))
    with np.errstate(all="ignore"):
        e1, e2 = b - a, c - a
        cx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
        cy = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
        cz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
        A = 0.5 * np.sqrt((cx * cx + cy * cy) + cz * cz)
    A[bad] = 0.0
    degenerate = ~bad & ~((A > 0.0) & (A < np.inf))
    A[degenerate] = 0.0
    return A, bad, degenerate


def quantum_exponent(amax, F):
    """(e, the mantissa of amax): frexp(amax) = (m, x), e = 61 - bit_length(F) - x (x = 0 for amax = 0)."""
    m, x = np.frexp(np.float64(amax))
    return 61 - int(F).bit_length() - int(x), float(m)


def quanta(A):
    """(q uint64 [F], e): q_f = floor(ldexp(A_f, e))."""
    A = np.asarray(A, np.float64)
    e, _ = quantum_exponent(A.max(), A.shape[0])
    with np.errstate(under="ignore"):
        q = np.floor(np.ldexp(A, e))
    assert (q < 2.0 ** (61 - int(A.shape[0]).bit_length())).all()
    return q.astype(np.uint64), e


def draw(vertices, faces, q, count, seed):
    """The samples for a table of quanta q (uint64 [F]): dict(face_index int64 [count], points float32 [count,3], u, v float64 [count]
    after the fold, total int); total == 0: None for all four (no point is written)."""
    v, f = np.asarray(vertices, np.float32), np.asarray(faces, np.int64).reshape(-1, 3)
    cum = np.cumsum(np.asarray(q, np.uint64), dtype=np.uint64)
    total = int(cum[-1])
    if total == 0:
        return dict(face_index=None, points=None, u=None, v=None, total=0)
    i = np.arange(int(count), dtype=np.uint32)
    k = [keys(seed, DRAW0 + d, i) for d in range(4)]
    t = np.array([(total * ((int(a) << 32) | int(b))) >> 64 for a, b in zip(k[0], k[1])], np.uint64)
    face = np.searchsorted(cum, t, side="right")  # the first f with cum[f] > t
    u, w = k[2].astype(np.float64) * 2.0 ** -32, k[3].astype(np.float64) * 2.0 ** -32
    fold = u + w > 1.0
    u, w = np.where(fold, 1.0 - u, u), np.where(fold, 1.0 - w, w)
    a, b, c = (v[f[face, j]].astype(np.float64) for j in range(3))
    p = a + ((b - a) * u[:, None] + (c - a) * w[:, None])
    return dict(face_index=face.astype(np.int64), points=p.astype(np.float32), u=u, v=w, total=total)


def sample_surface_oracle(vertices, faces, count, seed=0):
    """The whole rule: dict(points, face_index, keep uint8 [count], header int [8], q, e, A)."""
    A, bad, degenerate = face_areas(vertices, faces)
    q, e = quanta(A)
    d = draw(vertices, faces, q, count, seed)
    n = int(count) if d["total"] else 0
    header = [n, A.shape[0], int(bad.sum()), int(degenerate.sum()), e, d["total"] & MASK, d["total"] >> 32, 0]
    keep = np.full((int(count),), 1 if n else 0, np.uint8)
    return dict(points=d["points"], face_index=d["face_index"], keep=keep, header=header, q=q, e=e, A=A, u=d["u"], v=d["v"])


def header_i32(header):
    """The header as the device holds it: eight int32 (the total's words wrap)."""
    return np.array([int(x) & MASK for x in header], np.uint32).view(np.int32)
