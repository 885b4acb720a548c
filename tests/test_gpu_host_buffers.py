"""What a synchronous host-pointer entry point does with its caller's buffers must not show in its results: every one-chunk entry
point (and msiren_memcpy_h2d / _d2h) is called with the same data in buffers that are (a) pageable, (b) wholly page-locked and
(c) page-locked in part, and every output has to agree bit for bit between the three -- optional outputs given and omitted.  The calls
go through ctypes with explicit output arrays (np.empty is what pin_outputs(False) hands out, pinned_empty what pin_outputs(True) does),
so that windows of the caller's own arrays can be passed for (c).

(c) follows test_buffers_page_locked_in_part_go_through_a_bounce_buffer (test_gpu_parity.py): the CALLER registers the first half of one
fresh-page input arena and of one output arena with hipHostRegister, once for the whole module and from the main thread, and unregisters
them at the end; the calls get windows that straddle the registered edge.  One edge per arena: one input and one output of a call are
page-locked in part at a time, the call's other buffers are pageable, and the call is repeated until every buffer has had its turn.

Shapes: 17 tiles (one full 16-row prologue block and a ragged one), 50 coordinates (one full 32-chunk and a ragged one, under the
64-chunk), two 64 x 48 slices, 40 points, a ragged set of 70 coordinates over 5 patches of which one is empty.
"""
import ctypes as C

import numpy as np
import pytest

from mri_inr_amd import _lib, synthetic as syn
from test_gpu_parity import _fresh_pages, _range_kind, make_model

pytestmark = pytest.mark.gpu

B, Q, N, HH, WW, M, T, NP = 17, 50, 2, 64, 48, 40, 70, 5
L, H, Z, S = 5, 256, 256, 24
ARENA = 1 << 20          # bytes of either arena; the first half is registered
EDGE = ARENA // 2
KIND = {"pageable": 0, "pinned": 1, "partial": 2}

_rng = np.random.default_rng(7)
TILES = _rng.random((B, 32, 32), dtype=np.float32)
LATENT = _rng.normal(0.0, 0.5, (B, Z)).astype(np.float32)
MODS = syn.make_mods(41, L, B, H)
COORDS = _rng.uniform(-1.1, 1.1, (Q, 2)).astype(np.float32)
IMAGES = np.stack([syn.make_slice(k, HH, WW, brain_mask=bool(k)) for k in range(N)])
IMAGES2 = (IMAGES + _rng.normal(0.0, 0.05, IMAGES.shape)).astype(np.float32)
POINTS = (_rng.uniform(0.0, 1.0, (M, 2)) * np.array([HH - 1, WW - 1])).astype(np.float32)
RCOORDS = _rng.uniform(-1.1, 1.1, (T, 2)).astype(np.float32)
OFFSETS = np.array([0, 20, 20, 33, 50, T], np.int32)   # patch 1 is empty
RMODS = syn.make_mods(42, L, NP, H)


class In:
    def __init__(self, a):
        self.a = np.ascontiguousarray(a)


class Out:
    def __init__(self, shape, dtype=np.float32):
        self.shape, self.dtype = tuple(shape), np.dtype(dtype)


def _cases():
    """name -> (entry point, arguments behind the handle): In = a caller's input, Out = a caller's output, None = an output left out."""
    o, g, r = Out((B, Q)), Out((2, B, Q)), Out((N, HH, WW))          # 64 / 16 x 48 / 16 patches: the reconstruction has the image's size
    r8, gr, gr8 = Out((N, HH // 2, WW // 2)), Out((2, N, HH, WW)), Out((2, N, HH // 2, WW // 2))
    img, pts, rag = (In(IMAGES), N, HH, WW), (In(POINTS), M), (In(RCOORDS), In(OFFSETS), In(RMODS), NP, T)
    return {
        "forward_mods": ("msiren_forward_mods", (In(MODS), B, Out((B, S, S)))),
        "forward_latent": ("msiren_forward_latent", (In(LATENT), B, Out((B, S, S)), None)),
        "forward_latent+mods": ("msiren_forward_latent", (In(LATENT), B, Out((B, S, S)), Out((L, B, H)))),
        "forward_tiles": ("msiren_forward_tiles", (In(TILES), B, Out((B, S, S)))),
        "encode_tiles": ("msiren_encode_tiles", (In(TILES), B, Out((B, Z)))),
        "modulate": ("msiren_modulate", (In(LATENT), B, Out((L, B, H)))),
        "encode_modulate_tiles": ("msiren_encode_modulate_tiles", (In(TILES), B, None, Out((L, B, H)))),
        "encode_modulate_tiles+latent": ("msiren_encode_modulate_tiles", (In(TILES), B, Out((B, Z)), Out((L, B, H)))),
        "score_images": ("msiren_score_images", (In(IMAGES), In(IMAGES2), N, HH, WW, Out((N, 3), np.float64))),
        "reconstruct_slices": ("msiren_reconstruct_slices", img + (r,)),
        "reconstruct_slices_scaled": ("msiren_reconstruct_slices_scaled", img + (8, r8)),
        "reconstruct_slices_grad": ("msiren_reconstruct_slices_grad", img + (16, None, gr)),
        "reconstruct_slices_grad+recon": ("msiren_reconstruct_slices_grad", img + (16, r, gr)),
        "reconstruct_slices_grad+recon@8": ("msiren_reconstruct_slices_grad", img + (8, r8, gr8)),
        "sample_mods": ("msiren_sample_mods", (In(COORDS), Q, In(MODS), B, o)),
        "sample_tiles": ("msiren_sample_tiles", (In(COORDS), Q, In(TILES), B, o)),
        "sample_grad_mods": ("msiren_sample_grad_mods", (In(COORDS), Q, In(MODS), B, None, g)),
        "sample_grad_mods+out": ("msiren_sample_grad_mods", (In(COORDS), Q, In(MODS), B, o, g)),
        "sample_grad_tiles": ("msiren_sample_grad_tiles", (In(COORDS), Q, In(TILES), B, None, g)),
        "sample_grad_tiles+out": ("msiren_sample_grad_tiles", (In(COORDS), Q, In(TILES), B, o, g)),
        "sample_ragged_mods": ("msiren_sample_ragged_mods", rag + (Out((T,)),)),
        "sample_ragged_grad_mods": ("msiren_sample_ragged_grad_mods", rag + (None, Out((2, T)))),
        "sample_ragged_grad_mods+out": ("msiren_sample_ragged_grad_mods", rag + (Out((T,)), Out((2, T)))),
        "resample_slices": ("msiren_resample_slices", img + pts + (Out((N, M)),)),
        "resample_slices_grad": ("msiren_resample_slices_grad", img + pts + (None, Out((2, N, M)))),
        "resample_slices_grad+out": ("msiren_resample_slices_grad", img + pts + (Out((N, M)), Out((2, N, M)))),
    }


CASES = _cases()


@pytest.fixture(scope="module")
def models():
    sd = syn.make_state_dict(seed=7, trained_like=True)
    return {p: make_model(sd, precision=p) for p in ("f16x3", "fp32")}


@pytest.fixture(scope="module")
def arenas(models):
    """(input arena, output arena) as bytes, the first half of each page-locked by the caller: once, single-threaded."""
    hip = C.CDLL("libamdhip64.so")
    pair = [_fresh_pages((ARENA // 4,)).view(np.uint8) for _ in range(2)]
    done = []
    try:
        for a in pair:
            assert hip.hipHostRegister(C.c_void_p(a.ctypes.data), C.c_size_t(EDGE), C.c_uint(0)) == 0
            done.append(a)
        yield pair
    finally:
        for a in done:
            assert hip.hipHostUnregister(C.c_void_p(a.ctypes.data)) == 0


def _buffer(m, kind, nbytes, arena):
    """nbytes of the given kind, as a uint8 array (8-byte aligned)."""
    if kind == "pageable":
        return np.empty(nbytes, np.uint8)
    if kind == "pinned":
        return m.pinned_empty(((nbytes + 3) // 4,)).view(np.uint8)[:nbytes]
    assert 16 <= nbytes <= EDGE
    lo = EDGE - max(8, nbytes // 2 // 64 * 64)      # a window across the registered edge
    return arena[lo:lo + nbytes]


def _call(m, fn, args, arenas, kind="pageable", partial=()):
    """One call with its buffers of `kind`; the buffers whose argument index is in `partial` are windows across the arenas' edges.
    -> the outputs, copied."""
    cargs, outs, keep = [], [], []
    for i, a in enumerate(args):
        if not isinstance(a, (In, Out)):
            cargs.append(a)
            continue
        k = "partial" if i in partial else kind
        shape, dtype = (a.a.shape, a.a.dtype) if isinstance(a, In) else (a.shape, a.dtype)
        raw = _buffer(m, k, int(np.prod(shape)) * dtype.itemsize, arenas[isinstance(a, Out)])
        arr = raw.view(dtype).reshape(shape)
        if isinstance(a, In):
            arr[...] = a.a
        else:
            raw[...] = 0xFF                             # (NaN in either float type: a call that does not write shows)
            outs.append(arr)
        assert _range_kind(m, arr) == KIND[k], (fn, i, k)
        keep.append(raw)
        cargs.append(arr.ctypes.data)
    _lib.check(getattr(m._lib, fn)(m._h, *cargs))
    return [o.copy() for o in outs]


def _same(got, want, what):
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        assert np.array_equal(a, b), (what, k)


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("prec", ["f16x3", "fp32"])
def test_outputs_do_not_depend_on_what_the_callers_buffers_are(models, arenas, prec, name):
    m = models[prec]
    fn, args = CASES[name]
    want = _call(m, fn, args, arenas)
    assert all(np.isfinite(w).all() for w in want)
    _same(_call(m, fn, args, arenas, kind="pinned"), want, "pinned")
    ins = [i for i, a in enumerate(args) if isinstance(a, In)]
    outs = [i for i, a in enumerate(args) if isinstance(a, Out)]
    for r in range(max(len(ins), len(outs))):
        part = tuple(ins[r:r + 1] + outs[r:r + 1])
        arenas[1][...] = 0xFF
        got = _call(m, fn, args, arenas, partial=part)
        _same(got, want, ("partial", part))
        if outs[r:r + 1]:                                # nothing but the window was written
            n = want[r].nbytes
            lo = EDGE - max(8, n // 2 // 64 * 64)
            assert (arenas[1][:lo] == 0xFF).all() and (arenas[1][lo + n:] == 0xFF).all()
    _same(_call(m, fn, args, arenas), want, "pageable, again")


@pytest.mark.parametrize("prec", ["f16x3", "fp32"])
def test_an_output_left_out_does_not_change_the_others(models, arenas, prec):
    m = models[prec]
    for name in ("forward_latent", "encode_modulate_tiles", "reconstruct_slices_grad", "sample_grad_mods", "sample_grad_tiles",
                 "sample_ragged_grad_mods", "resample_slices_grad"):
        twin = name + ("+mods" if name == "forward_latent" else "+latent" if name == "encode_modulate_tiles" else
                       "+recon" if name == "reconstruct_slices_grad" else "+out")
        for kind in ("pageable", "pinned"):
            alone, both = _call(m, *CASES[name], arenas, kind=kind), _call(m, *CASES[twin], arenas, kind=kind)
            assert len(alone) == 1 and len(both) == 2
            kept = both[0] if name == "forward_latent" else both[1]      # (forward_latent's optional output is its last)
            assert np.array_equal(alone[0], kept), (name, kind)


@pytest.mark.parametrize("prec", ["f16x3", "fp32"])
def test_memcpy_from_and_to_buffers_of_every_kind(models, arenas, prec):
    m = models[prec]
    d = m.device_array(TILES.shape)
    for kind in KIND:
        src = _buffer(m, kind, TILES.nbytes, arenas[0]).view(np.float32).reshape(TILES.shape)
        src[...] = TILES + np.float32(KIND[kind])
        dst = _buffer(m, kind, TILES.nbytes, arenas[1]).view(np.float32).reshape(TILES.shape)
        dst[...] = np.nan
        assert _range_kind(m, src) == KIND[kind] and _range_kind(m, dst) == KIND[kind]
        _lib.check(m._lib.msiren_memcpy_h2d(m._h, d.ptr, src.ctypes.data, TILES.nbytes))
        assert np.array_equal(d.numpy(), src)
        _lib.check(m._lib.msiren_memcpy_d2h(m._h, dst.ctypes.data, d.ptr, TILES.nbytes))
        assert np.array_equal(dst, src), kind


def test_a_flagged_call_downloads_its_second_result_into_buffers_of_every_kind(models, arenas):
    """msiren_sample_mods on the split-fp16 handle with a modulation row beyond what fp16 carries (65 504): the host-side domain check
    runs the exact-fp32 trunk at the call's coordinates and finishes the call a second time -- into a pageable output (downloaded again),
    a page-locked one (in place) and one page-locked in part (the bounce buffer copied back behind the second wait).  The fp32 handle's bits."""
    m, exact = models["f16x3"], models["fp32"]
    bad = MODS.copy()
    bad[:, 5, :] *= np.float32(1e5)
    args = (In(COORDS), Q, In(bad), B, Out((B, Q)))
    want = _call(exact, "msiren_sample_mods", args, arenas)
    assert np.isfinite(want[0]).all()

    def events():
        n = C.c_int64()
        _lib.check(m._lib.msiren_range_events(m._h, C.byref(n)))
        return n.value

    for kind, partial in (("pageable", ()), ("pinned", ()), ("pageable", (4,)), ("pageable", (2,))):
        e0 = events()
        _same(_call(m, "msiren_sample_mods", args, arenas, kind=kind, partial=partial), want, (kind, partial))
        assert events() == e0 + 1, "the recipe no longer leaves the fp16 domain"
    clean = (In(COORDS), Q, In(MODS), B, Out((B, Q)))
    e0 = events()
    _same(_call(m, "msiren_sample_mods", clean, arenas, kind="pinned"), _call(m, "msiren_sample_mods", clean, arenas), "clean")
    assert events() == e0
