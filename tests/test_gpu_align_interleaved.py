"""The geometry calls of one handle share one block of their stream's scratch, laid out per call (mri_inr_amd/csrc/align_plan.h): bins, partial
records and, for a solve, its state behind them.  Here the eight kinds of call run on ONE handle in descending order of the scratch they need --
volume rigid solve, weighted affine solve with the intensity estimated, plain rigid solve, volume cost, weighted cost, plain cost,
resample_volume_with_gradient, resample_with_gradient -- so each finds the block as a larger call left it, and then twice in the reverse
order, so each also finds it as a smaller call left it.  Every result, traces included, must be the first pass's bit for bit: a stale
section, or a memset sized for another family, would show as a difference.  No tolerance: there is none to give.

Shapes: the case modules' smallest solve shapes (tests/align_solve_cases.py, align_w_cases.py, align_volume_cases.py: SOLVE_SHAPE, SOLVE_M) on
tests/volume_cases.py's stack; the points are volume_cases.make_points(0), the plain resample takes the (Y, X) of the first 200.
"""
import numpy as np
import pytest

import align_solve_cases as sc
import align_volume_cases as avc
import align_w_cases as wc
import test_gpu_align_solve as plain
import test_gpu_align_solve_w as weighted
import test_gpu_align_volume_solve as volume
import volume_cases as vc
from mri_inr_amd import align
from test_gpu_align import model

pytestmark = pytest.mark.gpu

NAME, PREC = "sine5", "fp32"


def calls(m):
    images, points = vc.images(), vc.make_points(0)[0]
    tg, tgw, tgv = plain.targets(NAME, PREC), weighted.targets(NAME, PREC), volume.targets(NAME, PREC)
    assert tgv.shape == (avc.SOLVE_M,) + avc.SOLVE_SHAPE and tg.shape == tgw.shape == (sc.N,) + sc.SHAPE
    return [("volume rigid solve", lambda: volume.solve(m, tgv, align.RIGID, trace=True)),
            ("weighted affine solve, intensity estimated", lambda: weighted.solve(m, tgw, align.AFFINE, align.ESTIMATE, trace=True)),
            ("plain rigid solve", lambda: plain.solve(m, tg, align.RIGID, trace=True)),
            ("volume cost", lambda: m.align_volume_cost(images, tgv, avc.start_maps(), warped=True, gradient=True)),
            ("weighted cost", lambda: m.align_cost_w(images, tgw, sc.start_maps(), weights=wc.solve_weights(), intensity=wc.start_intensity(align.ESTIMATE),
                                                     warped=True, gradient=True)),
            ("plain cost", lambda: m.align_cost(images, tg, sc.start_maps(), warped=True, gradient=True)),
            ("resample_volume_with_gradient", lambda: m.resample_volume_with_gradient(images, points)),
            ("resample_with_gradient", lambda: m.resample_with_gradient(images, points[:200, 1:]))]


def arrays(res):
    """a result (a namedtuple or tuple of arrays, scalars and Nones, or one array) as a flat list"""
    if isinstance(res, tuple):
        return [a for x in res for a in arrays(x)]
    return [None if res is None else np.asarray(res)]


def test_every_call_repeats_its_bits_whatever_ran_before_it():
    todo = calls(model(NAME, PREC))
    first = [arrays(fn()) for _, fn in todo]  # descending scratch
    assert all(any(a is not None and a.size for a in got) for got in first)
    assert first[0][-1] is not None and first[1][-3] is not None and first[2][-1] is not None, "the solves' traces are compared too"
    for rnd in range(2):  # ascending scratch, twice
        for (what, fn), want in reversed(list(zip(todo, first))):
            got = arrays(fn())
            assert len(got) == len(want), what
            for k, (a, b) in enumerate(zip(got, want)):
                assert (a is None) == (b is None), (what, rnd, k)
                assert a is None or (a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)), (what, rnd, k)
