"""The cases of msiren_residual_scale shared by tests/test_residual_scale_reference.py (CPU) and tests/test_gpu_residual_scale.py.
Not a test module; no GPU and no model needed: pure numpy, small enough that every GPU test takes seconds.

    LATTICES    19 x 23 and 33 x 37, the family's own, and 97 x 131 = 12 707 pixels: four chunks of 4096 with a ragged tail, not a multiple of 64
    KINDS       the residual arrays, M = 6 targets each, built from uint32 views where the bits matter: smooth noise; all values equal; exactly two
                distinct values; one array per key byte whose values differ in that byte only (that digit's pass alone decides the rank); denormals;
                +-0 mixed; large negatives with a few large positives (centre = 1: the deviations overflow to +inf at the top ranks); scattered +-inf
                and NaN; and `sparse`: a target with no pixel that counts, one with exactly one, one with exactly two, one with exactly 101 (quantile
                0.29: 0.29 100 = 28.999999999999996 in fp64, which floors to 28)
    weights     None, or a mask with 0, -1, NaN and +inf (none of which count) and a denormal (which counts) among ordinary weights
    SETTINGS    quantile x centre x groups at floor 0, and a floor above every s but the overflowing case's, once per centre
    GROUPS      None (singletons), (3, 1, 2), pooled
    many        258 targets of 5 x 7 and 1030 of 2 x 3: more segments than one workgroup of the last kernel has threads, more than two upload batches"""
import functools
import itertools

import numpy as np

from mri_inr_amd import residual_scale as rs

M = 6
LATTICES = ((19, 23), (33, 37), (97, 131))
KINDS = ("smooth", "equal", "two", "byte0", "byte1", "byte2", "byte3", "denormals", "zeros", "negatives", "nonfinite", "sparse")
QUANTILES = (0.0, 0.5, 1.0, 0.29)
GROUPS = (None, (3, 1, 2), (M,))
HIGH_FLOOR = 1e12
SETTINGS = tuple(dict(quantile=q, centre=c, groups=g, floor=0.0) for q, c, g in itertools.product(QUANTILES, (False, True), GROUPS)) + tuple(
    dict(quantile=0.5, centre=c, groups=None, floor=HIGH_FLOOR) for c in (False, True))
TUNE = 6 * rs.MAD_TO_SIGMA
HUNDRED_ONE = 3  # the target of `sparse` with exactly 101 pixels that count


def _from_bits(bits, shape):
    return np.ascontiguousarray(bits, dtype=np.uint32).view(np.float32).reshape(shape)


@functools.lru_cache(maxsize=None)
def residuals(kind, shape):
    """-> (M, th, tw) float32, read-only"""
    th, tw = shape
    full = (M, th, tw)
    n = M * th * tw
    rng = np.random.default_rng([KINDS.index(kind), th, tw])
    if kind == "smooth":
        e = (rng.standard_normal(full) * np.array([0.1, 1.0, 3.0, 0.01, 30.0, 1.0]).reshape(M, 1, 1) + 0.25).astype(np.float32)
    elif kind == "equal":
        e = np.full(full, 0.75, np.float32)
    elif kind == "two":
        e = np.where(rng.random(full) < 0.37, np.float32(-1.5), np.float32(2.25)).astype(np.float32)
    elif kind.startswith("byte"):
        b = int(kind[4])  # the byte of the key, 3 = the first digit; exponent bits below 0xFF everywhere: every value is finite
        base = np.uint32([0x3F123456, 0x3F123456, 0x3F003456, 0x00123456][b] & ~(0xFF << (8 * b)))
        e = _from_bits(base | (rng.integers(0, 256, n).astype(np.uint32) << np.uint32(8 * b)), full)
    elif kind == "denormals":
        e = _from_bits(rng.integers(1, 0x800000, n).astype(np.uint32) | (rng.integers(0, 2, n).astype(np.uint32) << np.uint32(31)), full)
    elif kind == "zeros":
        e = _from_bits(rng.integers(0, 2, n).astype(np.uint32) << np.uint32(31), full)
    elif kind == "negatives":
        e = (-1e30 * (1.0 + rng.random(full))).astype(np.float32)
        e[rng.random(full) < 0.02] = np.float32(3e38)
        e[rng.random(full) < 0.02] = np.float32(-3e38)
    elif kind == "nonfinite":
        e = rng.standard_normal(full).astype(np.float32)
        pick = rng.random(full)
        e[pick < 0.05] = np.float32(np.nan)
        e[(pick >= 0.05) & (pick < 0.08)] = np.float32(np.inf)
        e[(pick >= 0.08) & (pick < 0.11)] = np.float32(-np.inf)
    elif kind == "sparse":
        e = rng.standard_normal(full).astype(np.float32)
        for q, keep in ((0, 0), (1, 1), (2, 2), (HUNDRED_ONE, 101)):
            flat = e[q].reshape(-1)
            flat[rng.permutation(th * tw)[keep:]] = np.float32(np.nan)
    else:
        raise KeyError(kind)
    assert e.dtype == np.float32 and e.shape == full
    e.setflags(write=False)
    return e


@functools.lru_cache(maxsize=None)
def mask(shape):
    """-> weights (M, th, tw) float32: about a tenth each of 0, -1, NaN, +inf and a denormal, ordinary weights elsewhere"""
    th, tw = shape
    rng = np.random.default_rng([77, th, tw])
    w = (0.25 + rng.random((M, th, tw))).astype(np.float32)
    pick = rng.random((M, th, tw))
    for lo, value in ((0.0, 0.0), (0.1, -1.0), (0.2, np.nan), (0.3, np.inf)):
        w[(pick >= lo) & (pick < lo + 0.1)] = np.float32(value)
    w[(pick >= 0.4) & (pick < 0.5)] = _from_bits(np.uint32([0x00000400]), (1,))[0]
    w.setflags(write=False)
    return w


def weights_of(shape):
    return (("none", None), ("mask", mask(shape)))


@functools.lru_cache(maxsize=None)
def pair(shape):
    """-> (targets, simulated, intensity): what the residual is formed from on the device, with NaN holes in the simulated images and some -0.0"""
    th, tw = shape
    rng = np.random.default_rng([91, th, tw])
    S = rng.standard_normal((M, th, tw)).astype(np.float32)
    T = (S * np.float32(1.1) + rng.standard_normal((M, th, tw)).astype(np.float32) * np.float32(0.05)).astype(np.float32)
    S[rng.random(S.shape) < 0.04] = np.float32(np.nan)
    S[rng.random(S.shape) < 0.02] = np.float32(-0.0)
    T[rng.random(S.shape) < 0.02] = np.float32(-0.0)
    gb = np.stack([1.0 + 0.1 * rng.standard_normal(M), 0.05 * rng.standard_normal(M)], axis=1).astype(np.float32)
    for a in (T, S, gb):
        a.setflags(write=False)
    return T, S, gb


def many(m, shape, seed):
    """-> (m, th, tw) float32 of smooth noise, every target on a scale of its own"""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((m,) + shape) * (0.5 + rng.random((m, 1, 1)) * 4.0)).astype(np.float32)


def chunks(count, size):
    return [(lo, min(lo + size, count)) for lo in range(0, count, size)]


def bits_equal(a, b):
    """the same shape, dtype and bit patterns: -0.0 is not +0.0, a NaN equals itself"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
