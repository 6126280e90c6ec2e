"""Single-term probes (tests/fp32_probe.py) through every accepted FP32 kernel form: each output is ONE product x * w, or exactly zero,
and must be within 4 * 2^-24 of it, for dense weights against a sparse input (every weight element covered) and for a dense input against
sparse weights (every input element covered). The 1e-4 parity tests cannot see a missing low plane, a skipped plane product or a plane
element packed to the wrong lane (at most 2^-17 per product, less after a dense reduction); these can. tests/test_fp32_probe_cpu.py proves
on the CPU that the same probes pass the correctly emulated scheme and the oracle and fail each injected defect.
Also here: the dense accumulation statistic against the oracle's naive f32 sum, and weights set a second time on a live op."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from anakin_amd import lib as L  # noqa: E402
from anakin_amd import saber as S  # noqa: E402
from oracle import oracle as O  # noqa: E402
from tests import fp32_probe as P  # noqa: E402

# every kernel-selection code the library might accept for an FP32 conv (tests/test_gpu_parity.py: _F32_CODES); refused ones are skipped
F32_CODES = [t | ((ks | (sh << 4)) << 8) | (11 << 16) for t in range(10) for ks in (1, 2) for sh in (0, 1, 2, 3)] + \
            [v | (13 << 16) for v in range(1, 9)] + [v | (14 << 16) for v in range(0, 5)] + \
            [t | (ks << 8) | (v << 16) for v in (1, 2) for t in range(6) for ks in (1, 2, 4)]


@pytest.fixture(scope="module", autouse=True)
def _device():
    L.require_device()  # fail loudly: no fallback path exists


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _nhwc(a):
    return np.ascontiguousarray(a.transpose(0, 2, 3, 1))


def _forms(op):
    """[(code, algo name)]: the selection the op starts with, then every code set_tile accepts, one per kernel name"""
    forms = [(L.load().saber_hip_conv2d_get_tile(op.h), op.algo())]
    seen = {op.algo()}
    for code in F32_CODES:
        try:
            op.set_tile(code)
        except L.SaberHipError:
            continue
        if op.algo() not in seen:
            seen.add(op.algo())
            forms.append((code, op.algo()))
    op.set_tile(forms[0][0])
    assert op.algo() == forms[0][1], (op.algo(), forms[0])
    return forms


def _weight_groups(sets, stem=False):
    """[(family, w, bias, [passes])]: consecutive passes that share their weights run under one set_weights"""
    groups = []
    for fam, ps in sets.items():
        P.assert_full_coverage(ps, stem=stem)
        for p in ps.passes:
            if groups and groups[-1][0] == fam and groups[-1][1] is p.w:
                groups[-1][3].append(p)
            else:
                groups.append((fam, p.w, p.bias, [p]))
    return groups


def _make_conv(geo, w, b, relu=False, layout=L.NHWC):
    N, H, W, C, K, k, pad, stride, dil = geo
    p = S.ConvParam(w, b, 1, (pad, pad), (stride, stride), (dil, dil), relu)
    return S.SaberConv2D(int8=False).init((N, C, H, W), p, L.F32, L.F32, in_layout=layout, out_layout=layout)


def _probe_conv_forms(name, conv, disp, forms, sets, nchw=False):
    """every form x every pass of both families; the weights of a group are set on the LIVE op (the selection must survive that)"""
    xd = {}
    runs = 0
    for fam, w, b, passes in _weight_groups(sets, stem=name.startswith("stem/")):
        conv.set_weights(w, b)
        for code, algo in forms:
            conv.set_tile(code)
            assert conv.algo() == algo, (conv.algo(), algo)
            for p in passes:
                if id(p) not in xd:
                    xd[id(p)] = dev(p.x if nchw else _nhwc(p.x))
                y = disp.new_output()
                y.fill_(float("nan"))
                disp.dispatch(xd[id(p)], y)
                got = host(y)
                p.check(got if nchw else got.transpose(0, 3, 1, 2), "%s, %s probes, %s (%s)" % (name, fam, algo, hex(code)))
                runs += 1
    return runs


_CONV_CASES = [n for n in sorted(P.case_list()) if n.split("/")[0] in ("conv", "bias", "scale")]


@pytest.mark.parametrize("name", _CONV_CASES)
def test_conv_f32_single_term_probes_every_accepted_form(name):
    """Weight probes and activation probes, full coverage, through the static selection and every accepted selection code: 4 u."""
    geo = P.case_list()[name][0]
    sets = P.build_case(name)
    p0 = next(iter(sets.values())).passes[0]
    nchw = name.endswith("_nchw")
    conv = _make_conv(geo, p0.w, p0.bias, layout=L.NCHW if nchw else L.NHWC)
    forms = _forms(conv)
    runs = _probe_conv_forms(name, conv, conv, forms, sets, nchw=nchw)
    print("%s %s: %d kernel forms, %d probe launches within %g u: %s" % (name, geo, len(forms), runs, P.BOUND_U, " ".join(a for _, a in forms)))


def test_conv_f32_probe_geometries_reach_every_form_family():
    """The geometries above reach every family of FP32 kernels (the forms are enumerated exactly as the probe test enumerates them)."""
    seen = set()
    rng = np.random.default_rng(3)
    for name, geo in P.CONV_GEOMETRIES.items():
        N, H, W, C, K, k, pad, stride, dil = geo
        w = rng.standard_normal((K, C, k, k)).astype(np.float32)
        conv = _make_conv(geo, w, None, layout=L.NCHW if name.endswith("_nchw") else L.NHWC)
        seen |= {a for _, a in _forms(conv)}
    igemm = [a for a in seen if a.startswith("igemm_f32_bf16x3")]
    halo1 = [a for a in seen if a.startswith("pw1x1_f32_bf16x3_") and "_regs_" not in a and "_ksplit4_" not in a]
    want = {
        "bf16-plane implicit GEMM without split-K": [a for a in igemm if "_split" not in a],
        "bf16-plane implicit GEMM with split-K": [a for a in igemm if "_split" in a],
        "8-wave tile": [a for a in igemm if "_w8" in a],
        "halo 3x3": [a for a in seen if a.startswith("halo3x3_f32_bf16x3")],
        "halo 1x1": halo1,
        "register-weights pointwise": [a for a in seen if a.startswith("pw1x1_f32_bf16x3_regs_")],
        "reduction-split pointwise": [a for a in seen if a.startswith("pw1x1_f32_bf16x3_ksplit4_")],
        "f32 MFMA": [a for a in seen if a.startswith("igemm_f32_") and "bf16x3" not in a],
    }
    print({k: len(v) for k, v in want.items()})
    assert all(want.values()), {k: len(v) for k, v in want.items()}


@pytest.mark.parametrize("name", sorted(n for n in P.case_list() if n.startswith("pool2/")))
def test_conv_f32_relu_maxpool2x2_single_term_probes(name):
    """conv + relu + 2x2 / 2 max pooling in one launch (implicit GEMM and halo forms): the exact answer goes through relu and the pooling
    in float64, the probes are signed so that one term survives per window, the bound applies to the survivor."""
    geo = P.case_list()[name][0]
    N, H, W, C, K, k, pad, stride, dil = geo
    sets = P.build_case(name)
    p0 = sets["weight"].passes[0]
    cp = S.SaberConv2DPooling(int8=False).init((N, C, H, W), S.ConvParam(p0.w, None, 1, (pad, pad), (1, 1), (1, 1), True), L.POOL_MAX,
                                                (2, 2), (2, 2), (0, 0), L.F32, L.F32)
    assert cp.fused and cp.algo().endswith("+maxpool2x2"), cp.algo()
    forms = _forms(cp.conv)
    assert all(a.endswith("+maxpool2x2") for _, a in forms), forms
    assert any(a.startswith("halo3x3_f32_bf16x3") for _, a in forms) and any(a.startswith("igemm_f32_bf16x3") for _, a in forms), forms
    runs = _probe_conv_forms(name, cp.conv, cp, forms, sets)
    print("%s %s: %d kernel forms, %d probe launches within %g u" % (name, geo, len(forms), runs, P.BOUND_U))


@pytest.mark.parametrize("case", P.PAIR_GEOMETRIES)
def test_conv_f32_sibling_pair_single_term_probes(case):
    """Two FP32 convs over one input in one launch: the probes of the convolution with the K1 + K2 concatenated output channels, both outputs."""
    N, H, W, C, K1, K2, k, pad, stride = case
    name = "pair/%dx%dx%d_c%d_k%d+%d" % (N, H, W, C, K1, K2)
    sets = P.build_case(name)
    xd, runs, names = {}, 0, set()
    for fam, w, b, passes in _weight_groups(sets):
        a = _make_conv((N, H, W, C, K1, k, pad, stride, 1), w[:K1], None)       # (a pair copies its members' weights when it is created)
        c = _make_conv((N, H, W, C, K2, k, pad, stride, 1), w[K1:], None)
        pair = S.SaberConvPair(a, c)
        forms = _forms(pair)
        assert all(n.startswith("pair_") for _, n in forms), forms
        names |= {n for _, n in forms}
        for code, algo in forms:
            pair.set_tile(code)
            for p in passes:
                if id(p) not in xd:
                    xd[id(p)] = dev(_nhwc(p.x))
                ya, yb = a.new_output(), c.new_output()
                ya.fill_(float("nan"))
                yb.fill_(float("nan"))
                pair.dispatch(xd[id(p)], ya, yb)
                got = np.concatenate([host(ya), host(yb)], axis=3).transpose(0, 3, 1, 2)
                p.check(got, "%s, %s probes, %s" % (name, fam, pair.algo()))
                runs += 1
    print("%s: %d pair forms, %d probe launches within %g u" % (name, len(names), runs, P.BOUND_U))


@pytest.mark.parametrize("img", P.STEM_IMAGES)
def test_stem_f32_single_term_probes_all_tile_codes(img):
    """The FP32 stem launch (conv 7x7 / 2 + relu + max pooling 3x3 / 2 on the bf16 planes, NCHW image in): positive inputs, one positive
    weight per output channel, three weight sets so that each of the 147 (c, tap) positions is some channel's non-zero; all four tile codes.
    The weight sets after the first are set on the live op."""
    name = "stem/%dx%dx%d" % img
    N, H, W = img
    sets = P.build_case(name)
    assert len(sets["activation"].passes) >= 3
    p0 = sets["activation"].passes[0]
    stem = S.SaberConv2DPooling(int8=False).init((N, 3, H, W), S.ConvParam(p0.w, None, 1, (3, 3), (2, 2), (1, 1), True), L.POOL_MAX, (3, 3),
                                                  (2, 2), (0, 0), L.F32, L.F32, floor_mode=False, in_layout=L.NCHW)
    assert stem.fused and stem.algo() == "stem7x7s2_maxpool3x3s2_f32_bf16x3_nchw_in", stem.algo()
    forms = [((15 << 16) | v, stem.algo()) for v in range(4)]
    xd, runs = {}, 0
    for fam, w, b, passes in _weight_groups(sets, stem=True):
        stem.conv.set_weights(w, None)
        for code, algo in forms:
            stem.conv.set_tile(code)
            for p in passes:
                if id(p) not in xd:
                    xd[id(p)] = dev(p.x)
                y = stem.new_output()
                y.fill_(float("nan"))
                stem.dispatch(xd[id(p)], y)
                p.check(host(y).transpose(0, 3, 1, 2), "%s, tile code %s" % (name, hex(code)))
                runs += 1
    print("%s: 4 tile codes, %d probe launches within %g u" % (name, runs, P.BOUND_U))


def _gemm_probe(name, alpha, combos):
    geo = P.case_list()[name][0]
    M, _, _, Kd, Nc = geo[:5]
    sets = P.build_case(name)
    runs = 0
    for fam, w, b, passes in _weight_groups(sets):
        Bm = np.ascontiguousarray(w.reshape(Nc, Kd))          # [n][k]: trans_b's storage
        for ta, tb in combos:
            bd = dev(Bm if tb else Bm.T)
            for p in passes:
                A = p.x.reshape(M, Kd)
                c = torch.full((M, Nc), float("nan"), dtype=torch.float32, device="cuda")
                S.gemm(ta, tb, M, Nc, Kd, alpha, dev(A.T if ta else A), bd, 0.0, c)
                p.check(host(c).reshape(M, Nc, 1, 1), "%s, %s probes, trans_a %d trans_b %d alpha %g" % (name, fam, ta, tb, alpha))
                runs += 1
    return runs


@pytest.mark.parametrize("shape", P.GEMM_SHAPES)
def test_gemm_f32_single_term_probes(shape):
    """Gemm on the bf16 planes (k % 8 == 0; planes split on the device per call): A dense against one non-zero per column of B (every
    element of A covered) and one non-zero per row of A against dense B (every element of B covered), all four transpose combinations."""
    runs = _gemm_probe("gemm/%dx%dx%d" % shape, 1.0, [(0, 0), (0, 1), (1, 0), (1, 1)])
    print("gemm %s: %d probe launches within %g u" % (shape, runs, P.BOUND_U))


def test_gemm_f32_single_term_probes_with_alpha():
    """alpha = 0.7: the kernel rounds alpha * B to f32 before the split, so the exact answer is fl32(alpha * b) * a."""
    runs = _gemm_probe("gemm_alpha/%dx%dx%d" % P.GEMM_SHAPES[0], 0.7, [(0, 0), (0, 1), (1, 0), (1, 1)])
    print("gemm alpha 0.7: %d probe launches within %g u" % (runs, P.BOUND_U))


@pytest.mark.parametrize("splitk", [0, 1])
@pytest.mark.parametrize("shape", P.FC_SHAPES)
def test_fc_f32_single_term_probes(shape, splitk):
    """The FP32 fc kernels (f32 MFMA, no planes; the default kernel and the opt-in split-K one) under the same 4 u: dense input, one non-zero
    weight per output, with a bias."""
    M, K, N = shape
    name = "fc/%dx%dx%d" % shape
    sets = P.build_case(name)
    runs = 0
    for fam, w, b, passes in _weight_groups(sets):
        if splitk:
            os.environ["SABER_HIP_FC_F32_SPLITK"] = "1"      # opt-in, read by set_weights
        try:
            fc = S.SaberFc(False).init(M, N, K, np.ascontiguousarray(w.reshape(N, K)), b, L.F32)
        finally:
            os.environ.pop("SABER_HIP_FC_F32_SPLITK", None)
        assert fc.algo() == ("fc_f32_splitk_16xk4" if splitk else "fc_f32_small_16xk4"), fc.algo()
        for p in passes:
            y = torch.full((M, N), float("nan"), dtype=torch.float32, device="cuda")
            fc.dispatch(dev(p.x.reshape(M, K)), y)
            p.check(host(y).reshape(M, N, 1, 1), "%s, %s" % (name, fc.algo()))
            runs += 1
    print("%s %s: %d probe launches within %g u" % (name, fc.algo(), runs, P.BOUND_U))


# ---- dense inputs: the accumulation statistic ---------------------------------------------------------------------------------------------
# ratio = RMS(|got - exact| / sum|x||w|) of a kernel form / the same of the oracle's naive f32 convolution, measured on an MI355X for every
# form of the three geometries (DESIGN.md 4.8 has the table): the largest ratio per reduction length.
DENSE_MEASURED_MAX = {64: 0.972, 576: 0.986, 1152: 1.000}      # (the f32-MFMA forms; the bf16-plane forms: 0.31 - 0.78)


@pytest.mark.parametrize("length", sorted(P.DENSE_GEOMETRIES))
def test_conv_f32_dense_accumulation_statistic_vs_oracle(length):
    """Single-term probes say nothing about accumulation: for dense inputs (both signs, 12 binades) the RMS over the outputs of
    |got - exact64| / sum |x||w| of every form, relative to the oracle's. Asserted: ratio <= max(2, 1.5 x the largest measured) where that
    bound is below half the smallest emulated defect (tests/test_fp32_probe_cpu.py: DENSE_DEFECT_FLOOR); printed otherwise."""
    geo = P.DENSE_GEOMETRIES[length]
    N, H, W, C, K, k, pad, stride, dil = geo
    rng = np.random.default_rng(1000 + length)
    x, w = P.dense_inputs(geo, rng)
    exact, absum = P.dense_exact(geo, x, w)
    orc = P.dense_stat(O.conv_f32_nchw(x, w, None, False, (pad, pad)), exact, absum)
    conv = _make_conv(geo, w, None)
    xin = dev(_nhwc(x))
    measured = DENSE_MEASURED_MAX[length]
    bound = None if measured is None else max(2.0, 1.5 * measured)
    asserted = bound is not None and bound < 0.5 * P.DENSE_DEFECT_FLOOR[length]
    worst = 0.0
    forms = _forms(conv)
    for code, algo in forms:
        conv.set_tile(code)
        y = conv.new_output()
        conv.dispatch(xin, y)
        ratio = P.dense_stat(host(y).transpose(0, 3, 1, 2), exact, absum) / orc
        worst = max(worst, ratio)
        print("dense length %d %-44s ratio to the oracle %.3f" % (length, algo, ratio))
        if asserted:
            assert ratio <= bound, (length, algo, ratio, bound)
    print("dense length %d: oracle %.3f u, %d forms, largest ratio %.3f, bound %s (%s)" %
          (length, orc, len(forms), worst, bound, "asserted" if asserted else "printed only"))


# ---- weights set a second time ------------------------------------------------------------------------------------------------------------
_SET_WEIGHTS_CASES = {
    "register-weights pointwise": ("pw_c64_k256", (14 << 16) | 0, "pw1x1_f32_bf16x3_regs_"),
    "reduction-split pointwise": ("pw_c128_k512", (14 << 16) | 1, "pw1x1_f32_bf16x3_ksplit4_"),
    "halo 3x3": ("res2_3x3", (13 << 16) | 1, "halo3x3_f32_bf16x3_"),
    "split-K implicit GEMM": ("res4_3x3_n8", 2 | ((1 | (1 << 4)) << 8) | (11 << 16), "igemm_f32_bf16x3_"),
    "f32 MFMA implicit GEMM": ("c48_k34", 2 | (4 << 8) | (1 << 16), "igemm_f32_"),
}


@pytest.mark.parametrize("form", sorted(_SET_WEIGHTS_CASES) + ["stem"])
def test_conv_f32_weights_set_a_second_time(form):
    """saber_hip_conv2d_set_weights on a live op: weights A run, weights B (and another bias) set on the same op, and the op gives the bytes
    of a fresh op built with B under the same selection - also for the packings set_weights does not make itself (the stem launch's planes,
    the pointwise kernels' fragment-ordered planes); the selection stays."""
    rng = np.random.default_rng(len(form))
    if form == "stem":
        N, H, W = 2, 61, 47
        shape_w, code, prefix = (64, 3, 7, 7), (15 << 16) | 2, "stem7x7s2_maxpool3x3s2_f32_bf16x3"
        x = rng.uniform(-1, 1, (N, 3, H, W)).astype(np.float32)

        def make(w, b):
            op = S.SaberConv2DPooling(int8=False).init((N, 3, H, W), S.ConvParam(w, b, 1, (3, 3), (2, 2), (1, 1), True), L.POOL_MAX, (3, 3),
                                                        (2, 2), (0, 0), L.F32, L.F32, floor_mode=False, in_layout=L.NCHW)
            assert op.fused
            return op, op.conv
        xin = dev(x)
    else:
        gname, code, prefix = _SET_WEIGHTS_CASES[form]
        geo = P.CONV_GEOMETRIES[gname]
        N, H, W, C, K, k, pad, stride, dil = geo
        shape_w = (K, C, k, k)
        x = rng.standard_normal((N, C, H, W)).astype(np.float32)

        def make(w, b):
            op = _make_conv(geo, w, b)
            return op, op
        xin = dev(_nhwc(x))
    ws = [(rng.standard_normal(shape_w) * np.sqrt(2.0 / np.prod(shape_w[1:]))).astype(np.float32) for _ in range(2)]
    bs = [(rng.standard_normal(shape_w[0]) * 0.3).astype(np.float32) for _ in range(2)]

    def run(disp):
        y = disp.new_output()
        y.fill_(float("nan"))
        disp.dispatch(xin, y)
        return host(y)
    live, live_conv = make(ws[0], bs[0])
    live_conv.set_tile(code)
    name = live_conv.algo()
    assert name.startswith(prefix) and ("_split" in name) == form.startswith("split-K"), name
    ya = run(live)
    live_conv.set_weights(ws[1], bs[1])
    assert live_conv.algo() == name, (live_conv.algo(), name)
    yb = run(live)
    fresh, fresh_conv = make(ws[1], bs[1])
    fresh_conv.set_tile(code)
    assert fresh_conv.algo() == name
    want = run(fresh)
    assert np.isfinite(want).all() and not np.array_equal(ya, want)
    assert np.array_equal(yb, want), (form, name, float(np.abs(yb - want).max()), float(np.abs(yb - ya).max()))
    live_conv.set_weights(ws[0], bs[0])          # and back
    assert np.array_equal(run(live), ya), (form, name)
