"""The FP32 single-term probes (tests/fp32_probe.py) proven on the CPU: on every case the GPU probe test runs, the six-product bf16-plane
scheme emulated in numpy (both rounding models of the f32 accumulate) and the oracle's naive f32 convolution pass at 4 u with full coverage,
and the same emulation with one defect injected - the low plane of the weights zeroed, the mm product skipped, lh skipped, two elements of
a low plane swapped, the mid plane of one channel taken from its neighbour - FAILS. The bound is taken from the arithmetic and the
reference, not from a kernel; this file is the proof that it separates right from wrong."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import fp32_probe as P

CASES = sorted(P.case_list())


def _oracle(p):
    N, H, W, C, K, k, pad, stride, dil = p.geo
    y = O.conv_f32_nchw(p.x, p.w_exact, p.bias, p.relu, (pad, pad), (stride, stride), (dil, dil))
    if p.pool:
        win, st, ceil_mode = p.pool
        y = O.pool_f32_nchw(y, (win, win), (st, st), (0, 0), 0, floor_mode=not ceil_mode)
    return y


def _some(passes, n=3):
    """first, middle and last pass: the defects and the oracle need not run on every one of hundreds of passes"""
    idx = sorted({0, len(passes) // 2, len(passes) - 1})[:n]
    return [passes[i] for i in idx]


@pytest.mark.parametrize("name", CASES)
def test_correct_schemes_pass_with_full_coverage(name):
    sets = P.build_case(name)
    for fam, ps in sets.items():
        P.assert_full_coverage(ps, stem=name.startswith("stem/"))
        for i, p in enumerate(ps.passes):
            p.check(P.emulate(p, trunc=False), "%s %s pass %d, emulation (nearest)" % (name, fam, i))
            p.check(P.emulate(p, trunc=True), "%s %s pass %d, emulation (truncating)" % (name, fam, i))
        for p in _some(ps.passes):
            p.check(_oracle(p), "%s %s, oracle" % (name, fam))
        print("%s %s: %d passes, %d checked terms" % (name, fam, len(ps.passes), sum(len(p.term) for p in ps.passes)))


@pytest.mark.parametrize("name", CASES)
def test_every_injected_defect_fails(name):
    sets = P.build_case(name)
    for fam, ps in sets.items():
        for defect in (P.WEIGHT_SIDE if fam == "weight" else P.INPUT_SIDE):
            whole = defect in ("w_no_l", "no_mm", "no_lh")      # a defect of the scheme itself: most terms must show it, not a lucky few
            passes = _some(ps.passes) if whole else ps.passes   # (a packing slip of one element shows in the pass that covers that element)
            for trunc in ((False, True) if whole else (False,)):
                # (under a bias the bound is 4 u of |x w| + |b|: the single swapped pair sits in the channel with the smallest bias)
                bad = sum(len(p.failures(P.emulate(p, trunc=trunc, defect=defect, k0=0 if p.bias is None else int(np.abs(p.bias).argmin()))))
                          for p in passes)
                assert bad > 0, (name, fam, defect, trunc, "defect not detected")
                if whole:
                    total = sum(int((p.bound > 0).sum()) for p in passes)
                    assert bad > 0.5 * total, (name, fam, defect, trunc, bad, total)


def test_checker_wants_exact_zeros_and_rejects_nan():
    ps = P.build_case("conv/c16_dil2")["weight"]
    p = ps.passes[0]
    good = P.emulate(p)
    p.check(good)
    zero = np.argwhere(p.bound == 0)[0]
    for v in (1e-30, np.nan):
        g = good.copy()
        g[tuple(zero)] = v
        with pytest.raises(AssertionError):
            p.check(g)
    g = good.copy()
    g[tuple(zero)] = -0.0
    p.check(g)
    one = np.argwhere(p.bound > 0)[0]
    g = good.copy()
    g[tuple(one)] *= np.float32(1 + 2.0 ** -21)      # 8 u
    with pytest.raises(AssertionError, match="term w"):
        p.check(g)


def test_single_term_margins():
    """200 000 random products: the correct scheme stays below 4 u under both rounding models, the smallest defect is 30 x above it."""
    rng = np.random.default_rng(5)
    n = 200000
    idx, zero = np.arange(n), np.zeros(n, np.int64)
    worst = {}
    for vary_x in (True, False):       # n inputs against one weight, n weights against one input
        geo = P.gemm_geometry(n, 1, 1) if vary_x else P.gemm_geometry(1, n, 1)
        x, w = P.rand_f32(rng, (n if vary_x else 1, 1, 1, 1)), P.rand_f32(rng, (1 if vary_x else n, 1, 1, 1))
        p = P.Probe(geo, x, w, None, idx, idx if vary_x else zero, zero if vary_x else idx)
        for trunc in (False, True):
            for defect in (None, "w_no_l", "no_mm", "no_lh"):
                err = np.abs(P.emulate(p, trunc, defect).astype(np.float64) - p.exact) / np.abs(p.exact) / P.U
                worst[(defect, trunc)] = max(worst.get((defect, trunc), 0.0), float(err.max()))
    print(worst)
    assert worst[(None, False)] <= 2.0 and worst[(None, True)] <= 3.0
    assert min(worst[(d, t)] for d in ("w_no_l", "no_mm", "no_lh") for t in (False, True)) >= 100.0


@pytest.mark.parametrize("length", sorted(P.DENSE_GEOMETRIES))
def test_dense_statistic_of_the_emulated_schemes(length):
    """Dense accumulation: RMS of |got - exact| / sum |x||w| relative to the oracle's. The correct scheme (accumulating to nearest) is below
    the oracle's naive f32 sum; every whole-tensor defect is far above it. DENSE_DEFECT_FLOOR is what the GPU test's assertion refers to."""
    geo = P.DENSE_GEOMETRIES[length]
    rng = np.random.default_rng(1000 + length)
    x, w = P.dense_inputs(geo, rng)
    exact, absum = P.dense_exact(geo, x, w)
    N, H, W, C, K, k, pad, stride, dil = geo
    orc = P.dense_stat(O.conv_f32_nchw(x, w, None, False, (pad, pad)), exact, absum)
    good = P.dense_stat(P.emulate_dense(geo, x, w), exact, absum) / orc
    good_t = P.dense_stat(P.emulate_dense(geo, x, w, trunc=True), exact, absum) / orc
    bad = {d: P.dense_stat(P.emulate_dense(geo, x, w, defect=d), exact, absum) / orc for d in P.DENSE_DEFECTS}
    print("length %d: oracle %.3f u; ratio to the oracle: correct %.2f (truncating accumulate %.2f), defects %s" % (length, orc, good, good_t, bad))
    assert good <= 1.0
    assert min(bad.values()) >= P.DENSE_DEFECT_FLOOR[length]
