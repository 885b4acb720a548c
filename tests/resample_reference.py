"""Reference for the reconstruction at arbitrary points (msiren_resample_slices*): numpy, fp64, on top of
tests/grad_reference.value_and_grad.  Not a test module: tests/test_resample_reference.py checks it on the CPU, tests/test_gpu_resample.py
gates the kernels against it.

    pad = (S - I) / 2;  tile (v, h) covers (Y, X)  iff  v I - pad <= Y <= v I - pad + S - 1  and likewise for X   (closed; the fp32 Y is
                                                   compared with the exactly representable integers, no arithmetic on it)
    ty = Y - (v I - pad)          local coordinate  x_row = float32(-1 + ty 2 / (S - 1))          (same for columns)
    w  = float32(exp(-0.1 sqrt((ty - c)^2 + (tx - c)^2))),  c = (S - 1) / 2
    out  = sum_k w_k val_k / sum_k w_k            covering tiles in (v, h) row-major order; a black tile contributes 0 with its weight
    grad = (2 / (S - 1)) sum_k w_k g_k / sum_k w_k
A point without a covering tile (outside, or non-finite) is 0 / 0 = NaN.
"""
import numpy as np

import grad_reference as gr


def covering(y, n, S, I):
    """tiles of one axis that cover the fp32 coordinate y"""
    pad = (S - I) // 2
    y = np.float32(y)
    return [v for v in range(n) if np.float32(v * I - pad) <= y <= np.float32(v * I - pad + S - 1)]


def covers(points, nV, nH, S, I):
    """per point: [(tile, ty, tx), ...] in (v, h) row-major order, ty / tx in fp64"""
    pad = (S - I) // 2
    out = []
    for Y, X in np.asarray(points, dtype=np.float32):
        out.append([(v * nH + h, float(Y) - (v * I - pad), float(X) - (h * I - pad)) for v in covering(Y, nV, S, I) for h in covering(X, nH, S, I)])
    return out


def local_coord(t, S):
    return np.float32(-1.0 + np.asarray(t, dtype=np.float64) * 2.0 / (S - 1))


def weight(ty, tx, S):
    c = (S - 1) / 2
    return np.float32(np.exp(-0.1 * np.sqrt((np.asarray(ty, dtype=np.float64) - c) ** 2 + (np.asarray(tx, dtype=np.float64) - c) ** 2)))


def blend(points, nV, nH, S, I, tile_values, black=(), planes=1, dtype=np.float64):
    """(planes, M): ``tile_values(tile, ty, tx)`` -> (planes, count) are a tile's quantities at its entries (ty, tx: fp64 arrays)"""
    cov = covers(points, nV, nH, S, I)
    black = set(int(b) for b in black)
    per_tile = {}
    for m, lst in enumerate(cov):
        for k, (t, ty, tx) in enumerate(lst):
            per_tile.setdefault(t, []).append((m, ty, tx))
    num, den = np.zeros((planes, len(cov)), dtype), np.zeros(len(cov), dtype)
    for t in sorted(per_tile):  # (a point's tiles come up in ascending order: row-major, as the definition sums them)
        ms, ty, tx = (np.array(a) for a in zip(*per_tile[t]))
        ms = ms.astype(np.int64)
        w = weight(ty, tx, S).astype(dtype)
        den[ms] += w
        if t not in black:
            num[:, ms] += w * np.asarray(tile_values(t, ty, tx), dtype=dtype)
    with np.errstate(invalid="ignore", divide="ignore"):
        return num / den


def resample(sd, mods, black, points, nV, nH, S, I, *, num_layers, activation="sine", dtype=np.float64, perturbed=False):
    """One slice: mods (L, nV nH, H), one row per tile (the rows of black tiles are not read) -> (value (M), grad (2, M)), grad per
    reconstruction pixel.  dtype / perturbed as grad_reference.value_and_grad: fp32 + perturbed is the variant that sizes the gates."""
    t_ = np.dtype(dtype).type

    def tile_values(t, ty, tx):
        coords = np.stack([local_coord(ty, S), local_coord(tx, S)], axis=1)
        v, g = gr.value_and_grad(sd, mods[:, t:t + 1], coords, num_layers=num_layers, activation=activation, dtype=dtype, perturbed=perturbed)
        return np.concatenate([v, g[:, 0] * t_(2.0 / (S - 1))])

    out = blend(points, nV, nH, S, I, tile_values, black, planes=3, dtype=dtype)
    return out[0], out[1:]
