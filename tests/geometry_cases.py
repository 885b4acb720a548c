"""The point and alignment families (DESIGN.md sections 5.8 to 5.16) off the 3 x 3 square slice: geometries with nV != nH and with KA = ceil(S / I) =
1, 2, 3, 4 covering tiles per axis, their stacks, points, lattices, fp64 references and gates.  Not a test module; pure numpy plus the oracle, no GPU
needed: tests/test_geometry_reference.py checks on the CPU that the cases are what is said here and that the gates reject the transpositions they
are made for, tests/test_gpu_geometry.py gates the kernels.

    name   I   S   pad  KA  slices    tiles (nV, nH)          outer patch 32 throughout
    rect   16  24   4   2   40 x 72   (3, 5)
    ka3     8  24   8   3   40 x 56   (5, 7)
    ka4     8  32  12   4   40 x 56   (5, 7)
    ka1    32  32   0   1   40 x 72   (2, 3)                  covers do not overlap: a point strictly between two of them has no tile

The stack: n = 3 slices, synthetic.make_slice(3 + s).  Slice 1 has its leading I + (32 - I) / 2 COLUMNS zero: its tile column 0 is black (tiles
v nH, every v).  Slice 2 has as many leading ROWS zero: its tile row 0 is black (tiles 0 .. nH - 1).  A transposed black[] or pos lookup turns the one
into the other.  Models: sine5 everywhere, morlet3 on rect; state dicts of seed 7 built for the geometry's S.

The points (M ~ 340; ``parts`` names the index ranges):
    window_y   8 x 8 integer pixels across the seam of tile rows 0 | 1, in the core of the LAST tile column
    window_x   8 x 8 integer pixels across the seam of tile columns nH - 2 | nH - 1, in the core of the LAST tile row
    real       uniform over the whole cover
    ladder     (y_a, x_b) with exactly a and b covering tiles per axis, every 1 <= a, b <= KA (taken at the far end of each axis)
    edges      every exact cover edge v I - pad and v I - pad + S - 1 of both axes
    corners    the four cover corners of tile (nV - 1, 0) and of tile (0, nH - 1)
    pile       132 points in the core of one tile (rect (1, 3), ka3 and ka4 (2, 3), ka1 (1, 2)): its bin holds more than 128 entries, three chunks of 64
    between    (ka1) points strictly between two covers on each axis: NaN by the rule
    outside    just below / above the cover, far away, inf and NaN
Tile (0, 0) is left without a point (whatever falls into its cover is left out): the empty bin.  The volume forms take the same (Y, X) with Z
integer (windows, pile: Z = 1), fractional (real), on a cycle 0, 0.5, 1, 1.5, 2 (ladder, corners: Z = 0 and n - 1 among them), 1.5 (edges), and
six rows of invalid Z.

The lattices: tests/align_cases.py's maps and targets (their first n rows) and tests/align_volume_cases.py's targets 2, 3, 5 and 6 (ROWS3: the tilted
plane that crosses Z = 1 and leaves the stack above Z = 2, the one that leaves it below Z = 0, the anisotropic map that leaves every cover, the flat
plane whose target has NaN pixels; the fp64 reference of all seven would take the CPU 13 s on ka4), (19, 23) on every geometry and (47, 45) on rect,
every map's column offset moved by width - 28 so that the lattice lies across the slice's long axis and reads its last tile columns (on rect:
columns 3 and 4).  References and gates are the
existing ones (``*_of_stack``; gr.FACTOR / CAP_MAX / CAP_RMS on the planes, align_cases.FACTOR / CAP on the sums).
"""
import functools
from dataclasses import dataclass

import numpy as np

import align_cases as ac
import align_reference as ar
import align_robust_cases as rc
import align_robust_reference as arr
import align_volume_cases as avc
import align_volume_reference as avr
import align_volume_w_cases as vwc
import align_volume_w_reference as avwr
import align_w_cases as wc
import align_w_reference as awr
import grad_reference as gr
import resample_reference as rr
import volume_reference as vr
from mri_inr_amd import synthetic as syn
from oracle import siren_oracle as orc

O = 32
N = 3
EMPTY = (0, 0)


@dataclass(frozen=True)
class Geometry:
    name: str
    I: int
    S: int
    height: int
    width: int
    nV: int
    nH: int
    pile: tuple  # the tile whose core takes the pile

    @property
    def pad(self):
        return (self.S - self.I) // 2

    @property
    def KA(self):
        return -(-self.S // self.I)

    @property
    def K(self):
        return self.KA ** 2

    @property
    def NPt(self):
        return self.nV * self.nH

    @property
    def lo(self):
        return float(-self.pad)

    def hi(self, axis):
        """the last covered coordinate of axis 0 (Y) or 1 (X)"""
        return float(((self.nV, self.nH)[axis] - 1) * self.I - self.pad + self.S - 1)

    @property
    def shift(self):
        """what moves a lattice onto the slice's far columns"""
        return float(self.width - 28)


GEOMETRIES = {g.name: g for g in (Geometry("rect", 16, 24, 40, 72, 3, 5, (1, 3)), Geometry("ka3", 8, 24, 40, 56, 5, 7, (2, 3)), Geometry("ka4", 8, 32, 40, 56, 5, 7, (2, 3)),
                                  Geometry("ka1", 32, 32, 40, 72, 2, 3, (1, 2)))}
EXPECTED = {"rect": dict(pad=4, KA=2), "ka3": dict(pad=8, KA=3), "ka4": dict(pad=12, KA=4), "ka1": dict(pad=0, KA=1)}
MODELS = ac.MODELS
MODELS_OF = {"rect": ("sine5", "morlet3"), "ka3": ("sine5",), "ka4": ("sine5",), "ka1": ("sine5",)}
LATTICES_OF = {"rect": ((19, 23), (47, 45)), "ka3": ((19, 23),), "ka4": ((19, 23),), "ka1": ((19, 23),)}
COST_CASES = [(g, m, s) for g in GEOMETRIES for m in MODELS_OF[g] for s in LATTICES_OF[g]]


def tile(geo, v, h):
    return v * geo.nH + h


def black_tiles(geo):
    """what the docstring says of the three slices"""
    return [[], [tile(geo, v, 0) for v in range(geo.nV)], [tile(geo, 0, h) for h in range(geo.nH)]]


@functools.lru_cache(maxsize=None)
def state_dict(name, model="sine5"):
    return syn.make_state_dict(seed=7, num_layers=MODELS[model]["L"], siren_patch_size=GEOMETRIES[name].S, trained_like=True)


@functools.lru_cache(maxsize=None)
def images(name):
    geo = GEOMETRIES[name]
    img = np.stack([syn.make_slice(3 + s, geo.height, geo.width) for s in range(N)])
    dark = geo.I + (O - geo.I) // 2  # the outer patch of tile 0 of an axis ends there
    img[1, :, :dark] = 0.0
    img[2, :dark, :] = 0.0
    return img


@functools.lru_cache(maxsize=None)
def stack_mods(name, model, dtype_name):
    """per slice: the modulations of its tiles (rows of black tiles zero, never read) and its black tiles, as the oracle finds them"""
    geo, dtype, L, sd = GEOMETRIES[name], np.dtype(dtype_name).type, MODELS[model]["L"], state_dict(name, model)
    mods, black = [], []
    for img in images(name):
        patches, info = orc.image_to_patches(img, O, geo.I)
        kept, blk, _ = orc.filter_and_remember_black_patches(patches)
        assert info == (geo.nV, geo.nH), (name, info)
        m = np.zeros((L, geo.NPt, 256), dtype)
        z = orc.encoder_forward(sd, kept, dtype=dtype)
        m[:, [t for t in range(geo.NPt) if t not in blk]] = orc.modulator_forward(sd, z, num_layers=L, dtype=dtype)
        mods.append(m)
        black.append(list(blk))
    return mods, black


# ---- the points ---------------------------------------------------------------------------------------------------------------------------------
def in_tile(geo, p, v, h):
    """(Y, X) inside the cover of tile (v, h)"""
    lo_y, lo_x = v * geo.I - geo.pad, h * geo.I - geo.pad
    return (p[:, 0] >= lo_y) & (p[:, 0] <= lo_y + geo.S - 1) & (p[:, 1] >= lo_x) & (p[:, 1] <= lo_x + geo.S - 1)


def with_covers(geo, axis, a):
    """a coordinate of ``axis`` that exactly ``a`` tiles cover, at the far end of the axis"""
    return geo.hi(axis) - ((a - 1) * geo.I + 0.25)


def make_points(name, draw):
    """-> (points (M, 2) float32, parts: name -> slice)"""
    geo = GEOMETRIES[name]
    I, S, pad, nV, nH = geo.I, geo.S, geo.pad, geo.nV, geo.nH
    rng = np.random.default_rng(500 + draw)
    core = I // 2 - 4
    wy = np.stack(np.meshgrid(np.arange(I - 4, I + 4), (nH - 1) * I + core + np.arange(8), indexing="ij"), -1).reshape(-1, 2)
    wx = np.stack(np.meshgrid((nV - 1) * I + core + np.arange(8), np.arange((nH - 1) * I - 4, (nH - 1) * I + 4), indexing="ij"), -1).reshape(-1, 2)
    real = np.stack([rng.uniform(geo.lo, geo.hi(0), 200), rng.uniform(geo.lo, geo.hi(1), 200)], axis=1).astype(np.float32)
    real = real[~in_tile(geo, real, *EMPTY)][:40]
    ladder = np.array([[with_covers(geo, 0, a), with_covers(geo, 1, b)] for a in range(1, geo.KA + 1) for b in range(1, geo.KA + 1)])
    y_mid, x_mid = geo.hi(0) - S / 2 + 0.5, geo.hi(1) - S / 2 + 0.5
    edges = np.array([[v * I - pad + d, x_mid] for v in range(nV) for d in (0, S - 1)] + [[y_mid, h * I - pad + d] for h in range(nH) for d in (0, S - 1)])
    corners = np.array([[v * I - pad + dy, h * I - pad + dx] for v, h in ((nV - 1, 0), (0, nH - 1)) for dy in (0, S - 1) for dx in (0, S - 1)])
    pile = np.stack([rng.uniform(geo.pile[0] * I, geo.pile[0] * I + I - 1, 132), rng.uniform(geo.pile[1] * I, geo.pile[1] * I + I - 1, 132)], axis=1)
    between = np.array([[I - 0.5, x_mid], [y_mid, I - 0.5], [y_mid, (nH - 1) * I - 0.5], [I - 0.5, (nH - 1) * I - 0.5]]) if geo.KA == 1 else np.zeros((0, 2))
    below, above = np.nextafter(np.float32(geo.lo), np.float32(-np.inf)), np.nextafter(np.float32(geo.hi(1)), np.float32(np.inf))
    outside = np.array([[below, x_mid], [y_mid, above], [geo.hi(0) + 1, x_mid], [-40, 5], [5, 300], [np.inf, 3], [np.nan, x_mid]], np.float32)
    parts, rows, at = {}, [], 0
    for key, p in (("window_y", wy), ("window_x", wx), ("real", real), ("ladder", ladder), ("edges", edges), ("corners", corners), ("pile", pile),
                   ("between", between), ("outside", outside)):
        p = np.asarray(p, np.float32).reshape(-1, 2)
        if key not in ("between", "outside"):
            assert not in_tile(geo, p, *EMPTY).any(), (name, key)
        rows.append(p)
        parts[key] = slice(at, at + len(p))
        at += len(p)
    return np.concatenate(rows).astype(np.float32), parts


def make_points3(name, draw):
    """the same (Y, X) with a Z each, and six rows of invalid Z -> (points (M, 3) float32, parts)"""
    yx, parts = make_points(name, draw)
    rng = np.random.default_rng(700 + draw)
    z = np.zeros(len(yx), np.float32)
    cycle = np.array([0.0, 0.5, 1.0, 1.5, 2.0], np.float32)
    for key, sl in parts.items():
        count = sl.stop - sl.start
        z[sl] = (1.0 if key in ("window_y", "window_x", "pile") else rng.uniform(0.0, N - 1.0, count) if key == "real" else 1.5 if key == "edges" else
                 np.resize(cycle, count))
    pts = np.concatenate([z[:, None], yx], axis=1)
    geo = GEOMETRIES[name]
    y, x = geo.hi(0) - geo.S / 2 + 0.5, geo.hi(1) - geo.S / 2 + 0.5
    below, above = np.nextafter(np.float32(0), np.float32(-np.inf)), np.nextafter(np.float32(N - 1), np.float32(np.inf))
    invalid = np.array([[below, y, x], [-0.5, y, x], [above, y, x], [N, y, x], [np.nan, y, x], [np.inf, y, x]], np.float32)
    parts = dict(parts, invalid_z=slice(len(pts), len(pts) + len(invalid)))
    return np.concatenate([pts, invalid]).astype(np.float32), parts


def per_tile_counts(name, points):
    """covers per tile of a slice, as the bin kernels count them"""
    geo = GEOMETRIES[name]
    cov = rr.covers(points, geo.nV, geo.nH, geo.S, geo.I)
    return np.bincount([t for lst in cov for t, _, _ in lst], minlength=geo.NPt), [len(lst) for lst in cov]


def bin_counts3(name, points, value_form):
    """entries per (slice, tile) bin of the volume forms"""
    geo = GEOMETRIES[name]
    cov = rr.covers(points[:, 1:], geo.nV, geo.nH, geo.S, geo.I)
    counts = np.zeros(N * geo.NPt, np.int64)
    for lst, slices in zip(cov, vr.slices_read(points, N, value_form)):
        for s in slices:
            for t, _, _ in lst:
                counts[s * geo.NPt + t] += 1
    return counts


# ---- resample and resample_volume: reference, floor, gate ---------------------------------------------------------------------------------------------
def reference_slices(name, model, pts, dtype=np.float64, perturbed=False):
    """-> (value (n, M), grad (2, n, M)) of every slice at (Y, X)"""
    geo, mo = GEOMETRIES[name], MODELS[model]
    mods, black = stack_mods(name, model, np.dtype(dtype).name)
    out = [rr.resample(state_dict(name, model), mods[s], black[s], pts, geo.nV, geo.nH, geo.S, geo.I, num_layers=mo["L"], activation=mo["act"], dtype=dtype,
                       perturbed=perturbed) for s in range(N)]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out], axis=1)


def reference_volume(name, model, pts, dtype=np.float64, perturbed=False):
    geo, mo = GEOMETRIES[name], MODELS[model]
    mods, black = stack_mods(name, model, np.dtype(dtype).name)
    return vr.volume_of_stack(state_dict(name, model), mods, black, pts, geo.nV, geo.nH, geo.S, geo.I, num_layers=mo["L"], activation=mo["act"], dtype=dtype,
                              perturbed=perturbed)


def _drawn(name, model, make, reference, planes):
    """the first draw of 16 at most whose own floor (the reference's gradient in perturbed fp32 against itself in fp64) sits inside the caps"""
    for draw in range(16):
        pts, parts = make(name, draw)
        val, grad = reference(name, model, pts)
        v32, g32 = reference(name, model, pts, np.float32, perturbed=True)
        ok = np.isfinite(val if val.ndim == 1 else val[0])
        fm, fr = gr.distances(g32[planes][..., ok], grad[planes][..., ok])
        if gr.FACTOR * fm <= gr.CAP_MAX and gr.FACTOR * fr <= gr.CAP_RMS:
            break
    else:
        raise AssertionError(f"{name}: no draw of 16 inside the caps: last floor {fm:.2e} / {fr:.2e}")
    return dict(points=pts, parts=parts, value=val, grad=grad, finite=ok, draw=draw, floor=(fm, fr), value_floor=gr.distances(v32[..., ok], val[..., ok]),
                black=stack_mods(name, model, "float64")[1], gate=(min(gr.FACTOR * fm, gr.CAP_MAX), min(gr.FACTOR * fr, gr.CAP_RMS)))


@functools.lru_cache(maxsize=None)
def data(name, model="sine5"):
    """resample: points, parts, the fp64 reference of the n slices, the finite mask, the reference's own floor and the gradient gate"""
    return _drawn(name, model, make_points, reference_slices, slice(None))


@functools.lru_cache(maxsize=None)
def data3(name, model="sine5"):
    """resample_volume: as ``data``; the floor and the gate are those of the in-plane gradient grad[1:], as tests/volume_cases.py takes them"""
    return _drawn(name, model, make_points3, reference_volume, slice(1, None))


# ---- the mutants: the reference with one transposition or truncation planted --------------------------------------------------------------------------------
MUTANTS = ("tiles_h_nV_v", "cover_nV_nH_exchanged", "black_transposed", "slots_truncated", "pad_4")


def mutant_applies(name, mutant):
    geo = GEOMETRIES[name]
    return {"slots_truncated": geo.K > 4, "pad_4": geo.pad != 4}.get(mutant, geo.nV != geo.nH)


def mutant_slices(name, mutant, pts, model="sine5"):
    """reference_slices in fp64 with ``mutant`` planted in how a point finds its tiles:
        tiles_h_nV_v            the tile (its modulations and its black flag) indexed h nV + v
        cover_nV_nH_exchanged   the cover test runs over nH tile rows and nV tile columns (a tile row past nV - 1 has no tile: dropped)
        black_transposed        the black list alone read at h nV + v
        slots_truncated         a point's covers cut to the first min(K, 4) in row-major order
        pad_4                   the cover and the local coordinate formed with pad = 4"""
    geo, mo = GEOMETRIES[name], MODELS[model]
    nV, nH, S, I = geo.nV, geo.nH, geo.S, geo.I
    pad = 4 if mutant == "pad_4" else geo.pad
    rows, cols = (nH, nV) if mutant == "cover_nV_nH_exchanged" else (nV, nH)
    sd = state_dict(name, model)
    mods, black = stack_mods(name, model, "float64")

    def covering(y, n):
        y = np.float32(y)
        return [v for v in range(n) if np.float32(v * I - pad) <= y <= np.float32(v * I - pad + S - 1)]

    cov = []
    for Y, X in np.asarray(pts, np.float32):
        lst = [(v, h, float(Y) - (v * I - pad), float(X) - (h * I - pad)) for v in covering(Y, rows) for h in covering(X, cols) if v < nV and h < nH]
        cov.append(lst[:4] if mutant == "slots_truncated" else lst)
    val, grad = np.zeros((N, len(cov))), np.zeros((2, N, len(cov)))
    for s in range(N):
        per_tile = {}
        for m, lst in enumerate(cov):
            for v, h, ty, tx in lst:
                t = h * nV + v if mutant == "tiles_h_nV_v" else v * nH + h
                b = h * nV + v if mutant in ("tiles_h_nV_v", "black_transposed") else v * nH + h
                per_tile.setdefault((t, b in black[s]), []).append((m, ty, tx))
        num, den = np.zeros((3, len(cov))), np.zeros(len(cov))
        for (t, dark) in sorted(per_tile):
            ms, ty, tx = (np.array(a) for a in zip(*per_tile[(t, dark)]))
            ms = ms.astype(np.int64)
            w = rr.weight(ty, tx, S).astype(np.float64)
            den[ms] += w
            if not dark:
                coords = np.stack([rr.local_coord(ty, S), rr.local_coord(tx, S)], axis=1)
                v_, g_ = gr.value_and_grad(sd, mods[s][:, t:t + 1], coords, num_layers=mo["L"], activation=mo["act"], dtype=np.float64)
                num[:, ms] += w * np.concatenate([v_, g_[:, 0] * (2.0 / (S - 1))])
        with np.errstate(invalid="ignore", divide="ignore"):
            out = num / den
        val[s], grad[:, s] = out[0], out[1:]
    return val, grad


def outside_the_gate(d, val, grad, norm=(1e-4, 1e-5)):
    """what rejects a result of case ``d`` (from ``data``): the NaN pattern differs, the values miss the norm or the gradients miss the gate -> the reason, or None"""
    ok = d["finite"]
    if not (np.array_equal(np.isfinite(val), np.broadcast_to(ok, val.shape)) and np.array_equal(np.isfinite(grad), np.broadcast_to(ok, grad.shape))):
        return "nan pattern"
    vm, vrms = gr.distances(val[:, ok], d["value"][:, ok])
    gm, grms = gr.distances(grad[:, :, ok], d["grad"][:, :, ok])
    if vm > norm[0] or vrms > norm[1]:
        return f"values {vm:.1e} / {vrms:.1e}"
    if gm > d["gate"][0] or grms > d["gate"][1]:
        return f"gradients {gm:.1e} / {grms:.1e}"
    return None


# ---- the alignment cases ----------------------------------------------------------------------------------------------------------------------------
def maps2(name, shape):
    m = ac.maps(shape)[:N].copy()
    m[:, 5] += np.float32(GEOMETRIES[name].shift)
    return m


def targets2(shape):
    return ac.targets(shape)[:N]


def weights2(shape):
    return wc.weights(shape)[:N]


INTENSITY2 = wc.INTENSITY[:N]
ROWS3 = [2, 3, 5, 6]
M3 = len(ROWS3)
INTENSITY3, SCALE3 = vwc.INTENSITY[ROWS3], rc.SCALE[ROWS3]


def maps3(name, shape):
    m = avc.maps(shape)[ROWS3].copy()
    m[:, 8] += np.float32(GEOMETRIES[name].shift)
    return m


def targets3(shape):
    return avc.targets(shape)[ROWS3]


def weights3(shape):
    return vwc.weights(shape)[ROWS3]


def reference2(name, model, shape, dtype=np.float64, perturbed=False):
    geo, mo = GEOMETRIES[name], MODELS[model]
    mods, black = stack_mods(name, model, np.dtype(dtype).name)
    return ar.align_of_stack(state_dict(name, model), mods, black, maps2(name, shape), targets2(shape), geo.nV, geo.nH, geo.S, geo.I, num_layers=mo["L"],
                             activation=mo["act"], dtype=dtype, perturbed=perturbed)


def reference3(name, model, shape, dtype=np.float64, perturbed=False):
    geo, mo = GEOMETRIES[name], MODELS[model]
    mods, black = stack_mods(name, model, np.dtype(dtype).name)
    return avr.align_volume_of_stack(state_dict(name, model), mods, black, maps3(name, shape), targets3(shape), geo.nV, geo.nH, geo.S, geo.I,
                                     num_layers=mo["L"], activation=mo["act"], dtype=dtype, perturbed=perturbed)


def _case(sums, mags, s32, **kw):
    assert np.array_equal(s32[:, 0], sums[:, 0])  # the same pixels are valid
    D = float(ac.scaled_errors(s32, sums, mags).max())
    return dict(sums=sums, mags=mags, variant=s32, D=D, gate=min(ac.FACTOR * D, ac.CAP), **kw)


@functools.lru_cache(maxsize=None)
def align_data(name, model, shape):
    """-> the cases of align_cost ("plain") and align_cost_w ("w"): maps, targets, (weights, intensity), the fp64 sums, magnitudes and planes, D, gate"""
    sums, mags, planes = reference2(name, model, shape)
    s32, _, p32 = reference2(name, model, shape, np.float32, perturbed=True)
    base = dict(maps=maps2(name, shape), targets=targets2(shape), planes=planes)
    w = weights2(shape)
    sw, mw = awr.align(planes, base["targets"], w, INTENSITY2)
    s32w, _ = awr.align(p32, base["targets"], w, INTENSITY2)
    return dict(plain=_case(sums, mags, s32, **base), w=_case(sw, mw, s32w, weights=w, intensity=INTENSITY2, **base))


@functools.lru_cache(maxsize=None)
def align_volume_data(name, model, shape):
    """-> the cases of align_volume_cost ("plain"), align_volume_cost_w ("w") and align_volume_cost_r ("r")"""
    sums, mags, planes = reference3(name, model, shape)
    s32, _, p32 = reference3(name, model, shape, np.float32, perturbed=True)
    base = dict(maps=maps3(name, shape), targets=targets3(shape), planes=planes)
    w, gb = weights3(shape), INTENSITY3
    sw, mw = avwr.align(planes, base["targets"], w, gb)
    s32w, _ = avwr.align(p32, base["targets"], w, gb)
    sr, mr = arr.align(planes, base["targets"], w, gb, SCALE3)[:2]
    s32r = arr.align(p32, base["targets"], w, gb, SCALE3)[0]
    return dict(plain=_case(sums, mags, s32, **base), w=_case(sw, mw, s32w, weights=w, intensity=gb, **base),
                r=_case(sr, mr, s32r, weights=w, intensity=gb, scale=SCALE3, **base))


def accepts(d, sums):
    """the gate of a case on device sums: the count exact, every other sum within the gate on its scale"""
    sums = np.asarray(sums, np.float64)
    return bool(np.array_equal(sums[:, 0], d["sums"][:, 0]) and (ac.scaled_errors(sums, d["sums"], d["mags"]) <= d["gate"]).all())
