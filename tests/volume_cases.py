"""The stack and the points of tests/test_gpu_volume.py, with their fp64 reference.  Not a test module; no GPU
needed: tests/test_volume_reference.py checks on the CPU that a draw exists and that its bins are what is said here.

The stack: n = 4 slices of 40 x 40 (3 x 3 tiles each, the geometry of tests/test_gpu_resample.py); slice 1 has its rows :24 black (its
upper row of tiles is dropped by the plan), slice 3 is black altogether.  Bins are b = s 9 + t.
"""
import functools

import numpy as np

import grad_reference as gr
import volume_reference as vr
from mri_inr_amd import synthetic as syn
from oracle import siren_oracle as orc

O, I, S = 32, 16, 24
PAD = (S - I) // 2
NV = NH = 3
NPT = NV * NH
N = 4
L = 5
LO, HI = float(-PAD), float(NV * I - 1 + PAD)  # the cover of a whole slice: [-4, 51]
PILE_BIN = 2 * NPT + 4                         # (slice 2, tile (1, 1)): three chunks of 64
EMPTY_BINS = (0, 2 * NPT + 8, 3 * NPT + 8)     # the first, a middle and the last (slice, tile), in the value and the gradient forms


@functools.lru_cache(maxsize=None)
def full_sd():
    return syn.make_state_dict(seed=7, num_layers=L, trained_like=True)


@functools.lru_cache(maxsize=None)
def images():
    img = np.stack([syn.make_slice(3 + s, 40, 40) for s in range(N)])
    img[1, :24] = 0.0
    img[3] = 0.0
    return img


def in_tile(p, v, h):
    """(Y, X) inside the cover of tile (v, h)"""
    lo_y, lo_x = v * I - PAD, h * I - PAD
    return (p[:, 0] >= lo_y) & (p[:, 0] <= lo_y + S - 1) & (p[:, 1] >= lo_x) & (p[:, 1] <= lo_x + S - 1)


def keep_bins_empty(pts):
    """Z moved so that (slice 0, tile 0), (slice 2, tile 8) and (slice 3, tile 8) get no entry in either form: a point under tile (2, 2)
    reads slice 0 alone (Z = 0; the gradient forms add slice 1), a point under tile (0, 0) starts at slice 1"""
    pts = pts.copy()
    pts[in_tile(pts[:, 1:], 2, 2), 0] = 0.0
    low = in_tile(pts[:, 1:], 0, 0) & (pts[:, 0] < 1.0)
    pts[low, 0] += 1.0
    return pts


def make_points(draw):
    """M ~ 350 rows (Z, Y, X) and the index ranges of the parts"""
    rng = np.random.default_rng(300 + draw)

    def yx(count):
        return rng.uniform(LO, HI, size=(count, 2)).astype(np.float32)

    def with_z(z, p):
        return np.concatenate([np.broadcast_to(np.asarray(z, np.float32).reshape(-1, 1), (len(p), 1)), p], axis=1).astype(np.float32)

    window = with_z(2.0, np.stack(np.meshgrid(np.arange(10, 22), np.arange(10, 22), indexing="ij"), -1).reshape(-1, 2))  # integer pixels, integer Z
    frac = with_z(rng.uniform(0.0, 3.0, 60), yx(60))                                    # any Z
    per_segment = with_z(np.repeat([0.25, 1.5, 2.75], 6) + rng.uniform(-0.2, 0.2, 18), yx(18))
    whole = with_z(np.repeat([0.0, 1.0, 2.0, 3.0], 8), yx(32))                          # integer Z, Z = 0 and Z = n - 1 among them
    sixty4 = with_z(rng.integers(1, 192, 24) / 64.0, yx(24))                            # multiples of 1 / 64
    pile = with_z(2.0, rng.uniform(20.0, 27.0, size=(40, 2)).astype(np.float32))        # tile (1, 1) alone, slice 2 alone
    ends = [float(v * I - PAD + d) for v in range(NV) for d in (0, S - 1)]              # -4, 19, 12, 35, 28, 51
    edges = with_z(1.5, np.array([[e, 20.5] for e in ends] + [[20.5, e] for e in ends] + [[-4, -4], [51, 5], [19, 19], [12, 12], [35, 12]], np.float32))
    black = np.array([[3.0, 20.0, 20.0], [3.0, 5.5, 30.25], [1.0, 2.5, 20.0], [1.0, 7.0, 33.5], [2.5, 20.0, 20.0], [2.25, 14.5, 30.0]], np.float32)
    below, above = np.nextafter(np.float32(0), np.float32(-np.inf)), np.nextafter(np.float32(N - 1), np.float32(np.inf))
    invalid = np.array([[below, 20, 20], [-0.5, 20, 20], [above, 20, 20], [N, 20, 20], [np.nan, 20, 20], [np.inf, 20, 20],
                        [1.5, -10, 5], [1.0, 5, 100], [0.5, np.nextafter(np.float32(LO), np.float32(-np.inf)), 10], [1.5, np.nan, 7.5], [2.0, 3, np.inf]], np.float32)
    parts, rows, at = {}, [], 0
    for name, p in (("window", window), ("frac", frac), ("per_segment", per_segment), ("whole", whole), ("sixty4", sixty4), ("pile", pile),
                    ("edges", edges), ("black", black), ("invalid", invalid)):
        p = p if name in ("window", "pile", "black", "invalid") else keep_bins_empty(p)
        rows.append(p)
        parts[name] = slice(at, at + len(p))
        at += len(p)
    return np.concatenate(rows).astype(np.float32), parts


def bin_counts(points, value_form):
    """entries per (slice, tile) bin, as the bin kernels count them"""
    import resample_reference as rr

    cov = rr.covers(points[:, 1:], NV, NH, S, I)
    counts = np.zeros(N * NPT, np.int64)
    for lst, slices in zip(cov, vr.slices_read(points, N, value_form)):
        for s in slices:
            for t, _, _ in lst:
                counts[s * NPT + t] += 1
    return counts


@functools.lru_cache(maxsize=None)
def stack_mods(dtype_name):
    """per slice: the modulations of its tiles (rows of black tiles zero, never read) and its black tiles"""
    dtype = np.dtype(dtype_name).type
    sd = full_sd()
    mods, black = [], []
    for img in images():
        patches, info = orc.image_to_patches(img, O, I)
        kept, blk, _ = orc.filter_and_remember_black_patches(patches)
        assert info == (NV, NH)
        m = np.zeros((L, NPT, 256), dtype)
        if len(blk) < NPT:
            z = orc.encoder_forward(sd, kept, dtype=dtype)
            m[:, [t for t in range(NPT) if t not in blk]] = orc.modulator_forward(sd, z, num_layers=L, dtype=dtype)
        mods.append(m)
        black.append(list(blk))
    return mods, black


def reference(points, dtype=np.float64, perturbed=False, sub=slice(0, N)):
    mods, black = stack_mods(np.dtype(dtype).name)
    return vr.volume_of_stack(full_sd(), mods[sub], black[sub], points, NV, NH, S, I, num_layers=L, dtype=dtype, perturbed=perturbed)


@functools.lru_cache(maxsize=None)
def data():
    """The points -- the first draw, of 16 at most, at which the reference's own in-plane gradient in perturbed fp32 sits inside the caps, as
    tests/test_gpu_resample.py draws -- with the fp64 reference and the gate of grad[1:]: 4 x that distance, capped at the norm."""
    for draw in range(16):
        pts, parts = make_points(draw)
        val, grad = reference(pts)
        _, g32 = reference(pts, np.float32, perturbed=True)
        ok = np.isfinite(val)
        fm, fr = gr.distances(g32[1:, ok], grad[1:, ok])
        if gr.FACTOR * fm <= gr.CAP_MAX and gr.FACTOR * fr <= gr.CAP_RMS:
            break
    else:
        raise AssertionError(f"no draw of 16 inside the caps: last floor {fm:.2e} / {fr:.2e}")
    return dict(points=pts, parts=parts, value=val, grad=grad, finite=ok, black=stack_mods("float64")[1], draw=draw, floor=(fm, fr),
                gate=(min(gr.FACTOR * fm, gr.CAP_MAX), min(gr.FACTOR * fr, gr.CAP_RMS)))
