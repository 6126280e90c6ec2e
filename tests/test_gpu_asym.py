"""Per-axis convolution and pooling geometry on the GPU: kh != kw, pad_h != pad_w, stride_h != stride_w, dil_h != dil_w.

Every other suite gives both axes of a pair one value; here every case of tests/asym_util.py has H != W and a pair that differs, and
tests/test_asym_cpu.py proves that each case's oracle output changes when any such pair is swapped. Every kernel form the library accepts
for a case - the static selection and every selection code set_tile takes - must give the oracle's bytes (INT8) or stay within FP32_RTOL on
both criteria (FP32); so must the fused epilogues, the sibling pairs, the conv + pooling fusions, the pooling kernels and a hand-built
Inception-style net through the executor. The closing test asserts which kernel families were reached and that no accepted form was
skipped."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from anakin_amd import lib as L  # noqa: E402
from anakin_amd import saber as S  # noqa: E402
from oracle import oracle as O  # noqa: E402
from tests import asym_util as AU  # noqa: E402
from tests import guard_util as GU  # noqa: E402
from tests import int8_probe as P  # noqa: E402
from tests import test_gpu_guard as TG  # noqa: E402
from tests import test_gpu_parity as TP  # noqa: E402

FP32_RTOL = TP.FP32_RTOL
assert AU.I8_CODES == TP._I8_CODES and AU.F32_CODES == TP._F32_CODES      # (asym_util restates the lists for the host-side tests)

F32, S8, U8 = O.F32, O.S8, O.U8
NP_DT = {S8: np.int8, U8: np.uint8, F32: np.float32}
SENTINEL = 77
CASES = AU.ASYM_CONV_CASES
NAMES = sorted(CASES)
I8_COMBOS = list(P.CONV_COMBOS) + [(S8, F32, 0), (U8, F32, 1)]      # the probe suite's 8-bit combinations plus an f32 output

REACHED = {}        # family -> kernel names that ran and passed in this session
COUNTS = []         # (what, forms a descriptor-only handle accepts, forms run)


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


def _reach(family, name):
    REACHED.setdefault(family, set()).add(name)


def _forms(op, int8):
    return AU.accepted_forms(L.load(), op.h, AU.selection_codes(int8))


def _check_against_host(what, conv, ran, int8):
    """The forms run, against an enumeration that shares nothing with the op under test: a second handle made from the descriptor alone
    (no weights, no device buffers - the query of tests/test_asym_cpu.py) is walked through the same codes. INT8: the same kernel names.
    FP32: the bf16-plane forms exist only once set_weights has packed their planes, so the op under test runs the descriptor's forms
    plus bf16-plane ones, and nothing else."""
    import ctypes as C
    lib = L.load()
    h = C.c_void_p()
    assert lib.saber_hip_conv2d_create(C.byref(conv.desc), C.byref(h)) == 0, lib.saber_hip_last_error()
    host_names = {a for _, a in AU.accepted_forms(lib, h, AU.selection_codes(int8))}
    lib.saber_hip_conv2d_destroy(h)
    ran = set(ran)
    if int8:
        assert ran == host_names, (what, sorted(ran ^ host_names))
    else:
        assert host_names <= ran and all(a.startswith("igemm_f32_bf16x3_") for a in ran - host_names), (what, sorted(ran ^ host_names))
    COUNTS.append((what, len(host_names), len(ran)))


def _param(case, w, b, relu, ws=None):
    N, H, W, C, K, k, pad, stride, dil, g = case
    return S.ConvParam(w, b, g, pad, stride, dil, bool(relu), ws)


def _i8_conv(d, **kw):
    N, H, W, C = d.x.shape
    return S.SaberConv2D(True).init((N, C, H, W), _param(d.case, d.w, d.b, d.relu), d.idt, d.odt, d.in_scale, d.out_scale, **kw)


def _explain(got, want, alternatives):
    """the first differing element and, if any, the axis-swapped computation whose value it holds (called on a failure only)"""
    if got.shape != want.shape:
        return "shape %s, oracle %s" % (got.shape, want.shape)
    bad = np.argwhere(got != want)
    i = tuple(int(v) for v in bad[0])
    msg = "%d of %d differ, first at %s: got %s, oracle %s" % (len(bad), want.size, i, got[i], want[i])
    for label, fn in alternatives:
        alt = fn()
        if alt.shape == want.shape and alt[i] == got[i] and float(np.mean(alt == got)) > 0.9:
            msg += "; %.0f %% of the output equals the oracle computed with '%s'" % (100 * np.mean(alt == got), label)
    return msg


def _i8_alternatives(d):
    return [(label, (lambda how=how, pad=pad, stride=stride, dil=dil: d.oracle(wq=AU.swapped_weights(d.wq, how), pad=pad, stride=stride, dil=dil)))
            for label, how, pad, stride, dil in AU.swap_situations(d.case)
            if how != "transpose" and AU.situation_out_hw(d.case, how, pad, stride, dil) == d.want.shape[1:3]]


def _run_i8_forms(what, conv, d, family="conv_i8", res=None, prev=None, want=None):
    """every accepted form of an INT8 op into a sentinel-filled (or `prev`-filled) output: the oracle's bytes"""
    want = d.want if want is None else want
    x = dev(d.x)
    r = None if res is None else dev(res)
    forms = _forms(conv, True)
    ran = []
    for code, algo in forms:
        conv.set_tile(code)
        assert conv.algo() == algo, (conv.algo(), algo)
        y = conv.new_output()
        if prev is None:
            y.fill_(SENTINEL)
        else:
            y.copy_(dev(prev).view(y.dtype))
        conv.dispatch(x, y, r)
        got = host(y)
        assert got.dtype == want.dtype and got.shape == want.shape, (what, algo, got.shape, want.shape)
        if not np.array_equal(got, want):
            raise AssertionError("%s, %s (%s): %s" % (what, algo, hex(code), _explain(got, want, _i8_alternatives(d) if res is None and prev is None else [])))
        _reach(family, algo)
        ran.append(algo)
    _check_against_host(what, conv, ran, True)
    print("%s: %d kernel forms bit-exact: %s" % (what, len(ran), " ".join(ran)))
    return [a for _, a in forms]


def _f32_errors(got, want):
    d = np.abs(got - want)
    scale = max(float(np.abs(want).max()), 1e-6)
    return float(d.max() / scale), float((d / (np.abs(want) + np.abs(want).mean() + 1e-12)).max())


def _run_f32_forms(what, conv, x_dev, want, family="conv_f32", prev=None):
    """every accepted form of an FP32 op: both criteria of test_conv_f32_random_geometry_..., and the same bits on a second launch"""
    forms = _forms(conv, False)
    ran = []

    def run():
        y = conv.new_output()
        if prev is None:
            y.fill_(float(SENTINEL))
        else:
            y.copy_(dev(prev))
        conv.dispatch(x_dev, y)
        return host(y)
    for code, algo in forms:
        conv.set_tile(code)
        assert conv.algo() == algo, (conv.algo(), algo)
        got = run()
        assert got.shape == want.shape, (what, algo, got.shape, want.shape)
        e_max, e_el = _f32_errors(got, want)
        assert e_max <= FP32_RTOL and e_el <= FP32_RTOL, (what, algo, hex(code), e_max, e_el)
        assert np.array_equal(run(), got), ("not deterministic", what, algo)
        _reach(family, algo)
        ran.append(algo)
    _check_against_host(what, conv, ran, False)
    print("%s: %d kernel forms within 1e-4: %s" % (what, len(ran), " ".join(ran)))
    return [a for _, a in forms]


# ==== the table, INT8 ========================================================================================================================
@pytest.mark.parametrize("name", NAMES)
def test_int8_table_every_accepted_form_is_bit_exact(name):
    """two of the ten dtype / relu combinations per case (rotating), one with and one without bias; the static selection and every accepted
    code of the parity tests' list plus variants 16 / 17"""
    case, i = CASES[name], NAMES.index(name)
    for j, bias in ((i, True), (i + len(I8_COMBOS) // 2, False)):
        idt, odt, relu = I8_COMBOS[j % len(I8_COMBOS)]
        d = AU.I8Data(case, idt, odt, relu, bias, seed=AU.seed_of(name, j))
        conv = _i8_conv(d)
        assert conv.out_shape() == d.want.shape
        _run_i8_forms("i8 %s %s in %d out %d relu %d bias %d" % (name, case, idt, odt, relu, bias), conv, d)


# ==== the table, FP32 ========================================================================================================================
@pytest.mark.parametrize("layout", ["nhwc", "nchw"])
@pytest.mark.parametrize("name", NAMES)
def test_fp32_table_every_accepted_form_within_tolerance(name, layout):
    case = CASES[name]
    N, H, W, C, K, k, pad, stride, dil, g = case
    d = AU.F32Data(case, seed=AU.seed_of(name, 3), relu=True)
    lay = L.NCHW if layout == "nchw" else L.NHWC
    conv = S.SaberConv2D(False).init((N, C, H, W), _param(case, d.w, d.b, True), L.F32, L.F32, in_layout=lay, out_layout=lay)
    want = d.want if layout == "nchw" else _nhwc(d.want)
    names = _run_f32_forms("f32 %s %s %s" % (name, case, layout), conv, dev(d.x if layout == "nchw" else _nhwc(d.x)), want)
    # the bf16-plane halo and pointwise kernels (variants 13 / 14) and the depthwise kernels take no per-axis descriptor, weights set or not
    assert not any(a.startswith(("halo3x3_f32", "pw1x1_f32", "dw3x3")) for a in names), names
    if g > 1:
        assert set(names) == {"direct_f32"}, names


# ==== random per-axis geometry ===============================================================================================================
@pytest.mark.parametrize("seed", range(24))
def test_conv_i8_random_asym_geometry_every_accepted_selection_is_bit_exact(seed):
    """test_conv_i8_random_geometry_every_accepted_selection_is_bit_exact with every pair drawn per axis"""
    rng = np.random.default_rng(19000 + seed)
    case = AU.random_asym_geometry(rng, True)
    idt = int(rng.choice([S8, U8]))
    odt = int(rng.choice([S8, U8, F32]))
    relu = int(rng.integers(0, 2)) if odt != U8 else 1
    d = AU.I8Data(case, idt, odt, relu, True, seed=int(rng.integers(1 << 30)))
    d.in_scale, d.out_scale = float(rng.choice([0.017, 0.0039, 0.11])), float(rng.choice([0.041, 0.009, 0.3]))
    _run_i8_forms("i8 seed %d %s in %d out %d relu %d" % (seed, case, idt, odt, relu), _i8_conv(d), d)


@pytest.mark.parametrize("seed", range(16))
def test_conv_f32_random_asym_geometry_every_accepted_selection_within_tolerance(seed):
    """the FP32 twin: optional in-place residual sum + relu, NHWC"""
    rng = np.random.default_rng(17000 + seed)
    case = AU.random_asym_geometry(rng, False)
    N, H, W, C, K, k, pad, stride, dil, g = case
    elt = bool(rng.integers(0, 2))
    d = AU.F32Data(case, seed=int(rng.integers(1 << 30)), relu=not elt)
    want = _nhwc(d.want)
    res = (rng.random(want.shape) * 2.0).astype(np.float32) if elt else None
    p = _param(case, d.w, d.b, not elt)
    if elt:
        want = np.maximum(want + res, 0.0)
        p.res_mode, p.res_relu, p.sum_scale = L.RES_SUM_INPLACE, True, 1.0
    conv = S.SaberConv2D(False).init((N, C, H, W), p, L.F32, L.F32, in_layout=L.NHWC, out_layout=L.NHWC)
    _run_f32_forms("f32 seed %d %s%s" % (seed, case, " + sum" if elt else ""), conv, dev(_nhwc(d.x)), want, prev=res)


# ==== fused epilogues ========================================================================================================================
FUSED_CASES = ["k1x7", "s21"]


@pytest.mark.parametrize("name", FUSED_CASES)
@pytest.mark.parametrize("res_relu", [False, True])
def test_int8_fused_eltwise_on_per_axis_convs(name, res_relu):
    """RES_ELTWISE: conv (-> s8, no relu) + the INT8 eltwise sum with an s8 residual in one launch == the oracle's two ops"""
    case = CASES[name]
    d = AU.I8Data(case, U8, S8, 0, True, seed=AU.seed_of(name, 11 + res_relu))
    s_res, s_out = 0.043, 0.06
    c = float(np.float32(1.0 / s_out))
    res = np.random.default_rng(AU.seed_of(name, 12)).integers(-128, 128, d.want.shape).astype(np.int8)
    p = _param(case, d.w, d.b, 0)
    p.res_mode, p.res_relu, p.sum_scale, p.coeff, p.scale_res = L.RES_ELTWISE, res_relu, 1.0, (c, c), s_res
    conv = S.SaberConv2D(True).init((case[0], case[3], case[1], case[2]), p, U8, S8, d.in_scale, d.out_scale)
    want = O.eltwise_i8(d.want, res, d.out_scale, s_res, c, c, res_relu)
    assert (want != d.want).mean() > 0.5
    _run_i8_forms("i8 + eltwise %s relu %d" % (name, res_relu), conv, d, family="fused_i8", res=res, want=want)


@pytest.mark.parametrize("name", FUSED_CASES)
def test_int8_sum_inplace_on_per_axis_convs(name):
    """RES_SUM_INPLACE: s8 bytes already in a u8 output are summed in (the JIT post-op's order), scale != 1"""
    case = CASES[name]
    d = AU.I8Data(case, U8, U8, 1, True, seed=AU.seed_of(name, 13))
    ss = 0.61
    prev = np.random.default_rng(AU.seed_of(name, 14)).integers(-128, 128, d.want.shape).astype(np.int8)
    p = _param(case, d.w, d.b, 1)
    p.res_mode, p.res_relu, p.sum_scale, p.res_dtype = L.RES_SUM_INPLACE, False, ss, S8
    conv = S.SaberConv2D(True).init((case[0], case[3], case[1], case[2]), p, U8, U8, d.in_scale, d.out_scale)
    bp, sc = O.conv_i8_prepare(d.ws, d.b, d.in_scale, d.out_scale, U8, U8)
    want = O.conv_i8(d.x, d.wq, bp, sc, U8, 1, case[6], case[7], case[8], residual=O.Residual(O.RES_JIT_SUM, 0, ss, S8, 0, 0, 0, 0),
                     out_init=prev.view(np.uint8))
    assert (want != d.want).mean() > 0.3
    _run_i8_forms("i8 + sum in place %s" % name, conv, d, family="fused_i8", prev=prev.view(np.uint8), want=want)


@pytest.mark.parametrize("name", FUSED_CASES)
def test_fp32_sum_inplace_relu_on_per_axis_convs(name):
    case = CASES[name]
    N, H, W, C, K, k, pad, stride, dil, g = case
    d = AU.F32Data(case, seed=AU.seed_of(name, 15), relu=False)
    res = (np.random.default_rng(AU.seed_of(name, 16)).random(_nhwc(d.want).shape) * 2.0).astype(np.float32)
    p = _param(case, d.w, d.b, False)
    p.res_mode, p.res_relu, p.sum_scale = L.RES_SUM_INPLACE, True, 1.0
    conv = S.SaberConv2D(False).init((N, C, H, W), p, L.F32, L.F32, in_layout=L.NHWC, out_layout=L.NHWC)
    _run_f32_forms("f32 + sum + relu %s" % name, conv, dev(_nhwc(d.x)), np.maximum(_nhwc(d.want) + res, 0.0), family="fused_f32", prev=res)


# ==== sibling pairs ==========================================================================================================================
PAIR_CASES = {"k1x7": (1, 9, 13, 64, (1, 7), (0, 3), (1, 1)), "s12": (1, 12, 15, 64, (3, 3), (1, 1), (1, 2))}
PAIR_K = (128, 32)
I8_PAIR_CODES = [t | (ks << 8) | (1 << 16) for t in range(6) for ks in (1, 2, 4)] + [t | (4 << 8) | (2 << 16) for t in range(6)] + \
                [t | (4 << 8) | (3 << 16) for t in range(3)] + [0 | (4 << 8) | (4 << 16)]


@pytest.mark.parametrize("name", sorted(PAIR_CASES))
@pytest.mark.parametrize("idt", [U8, S8])
def test_int8_sibling_pair_on_per_axis_convs(name, idt):
    """two INT8 convs (K = 128 and 32) over one input in one launch: both outputs equal the two ops run alone and the oracle, in every form"""
    N, H, W, C, k, pad, stride = PAIR_CASES[name]
    x = AU.rand8(np.random.default_rng(AU.seed_of(name, 20 + idt)), (N, H, W, C), idt)
    convs, wants = [], []
    for n, (K, odt, relu) in enumerate(((PAIR_K[0], S8, 0), (PAIR_K[1], U8, 1))):
        d = AU.I8Data((N, H, W, C, K, k, pad, stride, (1, 1), 1), idt, odt, relu, True, seed=AU.seed_of(name, 22 + n))
        d.x = x
        wants.append(d.want)
        convs.append(_i8_conv(d))
    pair = S.SaberConvPair(convs[0], convs[1])
    assert pair.algo().startswith("pair_igemm_i8"), pair.algo()
    xd = dev(x)
    alone = []
    for c, w in zip(convs, wants):
        y = c.new_output()
        c.dispatch(xd, y)
        alone.append(host(y))
        assert np.array_equal(alone[-1], w), (name, c.algo())
    forms = AU.accepted_forms(L.load(), pair.h, I8_PAIR_CODES)
    for code, algo in forms:
        pair.set_tile(code)
        ya, yb = convs[0].new_output(), convs[1].new_output()
        ya.fill_(SENTINEL)
        yb.fill_(SENTINEL)
        pair.dispatch(xd, ya, yb)
        assert np.array_equal(host(ya), wants[0]) and np.array_equal(host(yb), wants[1]), (name, algo, hex(code))
        _reach("pair_i8", algo)
    assert len(forms) >= 20, forms
    print("pair i8 %s: %d forms" % (name, len(forms)))


F32_PAIR_CODES = [0 | (1 << 8) | (1 << 16), 2 | (2 << 8) | (1 << 16), 3 | (4 << 8) | (1 << 16), 5 | (1 << 8) | (1 << 16), 2 | (4 << 8) | (2 << 16),
                  1 | (4 << 8) | (3 << 16), 0 | (4 << 8) | (4 << 16)]


@pytest.mark.parametrize("name", sorted(PAIR_CASES))
def test_fp32_sibling_pair_on_per_axis_convs(name):
    """the FP32 pair: bit-identical to the two convs run alone with the same tile (same reduction order), within 1e-4 of the oracle"""
    N, H, W, C, k, pad, stride = PAIR_CASES[name]
    convs, wants = [], []
    x = None
    for n, (K, relu) in enumerate(((PAIR_K[0], False), (PAIR_K[1], True))):
        case = (N, H, W, C, K, k, pad, stride, (1, 1), 1)
        d = AU.F32Data(case, seed=AU.seed_of(name, 30), relu=relu)      # (the same seed: the same x, drawn first)
        x = d.x if x is None else x
        assert np.array_equal(x, d.x)
        d.w = (np.random.default_rng(AU.seed_of(name, 31 + n)).standard_normal(d.w.shape) * np.sqrt(2.0 / (C * k[0] * k[1]))).astype(np.float32)
        wants.append(_nhwc(d.oracle()))
        convs.append(S.SaberConv2D(False).init((N, C, H, W), _param(case, d.w, d.b, relu), L.F32, L.F32, in_layout=L.NHWC, out_layout=L.NHWC))
    xd = dev(_nhwc(x))
    pair = S.SaberConvPair(convs[0], convs[1])
    assert pair.algo().startswith("pair_igemm_f32"), pair.algo()
    forms = AU.accepted_forms(L.load(), pair.h, F32_PAIR_CODES)
    same_bits = 0
    for code, algo in forms:
        pair.set_tile(code)
        ya, yb = convs[0].new_output(), convs[1].new_output()
        ya.fill_(7.0)
        yb.fill_(7.0)
        pair.dispatch(xd, ya, yb)
        for c, got, want in zip(convs, (host(ya), host(yb)), wants):
            try:
                c.set_tile(code)      # the same tile and staging: the same reduction order
            except L.SaberHipError:
                pass
            if "pair_" + c.algo() == algo:
                y = c.new_output()
                c.dispatch(xd, y)
                assert np.array_equal(got, host(y)), (name, algo, c.algo())
                same_bits += 1
            e_max, e_el = _f32_errors(got, want)
            assert e_max <= FP32_RTOL and e_el <= FP32_RTOL, (name, algo, e_max, e_el)
        _reach("pair_f32", algo)
    assert same_bits >= 2 * (len(forms) - 1), (same_bits, forms)
    assert len(forms) >= 5, forms


# ==== conv + pooling in one launch ===========================================================================================================
@pytest.mark.parametrize("geo", [(2, 8, 12, 16, 24, (3, 1), (1, 0), (1, 1)), (1, 10, 12, 32, 40, (3, 3), (1, 1), (1, 2))])
def test_fp32_conv_relu_maxpool2x2_on_per_axis_convs(geo):
    """SaberConv2DPooling, FP32: 3x1 with pad (1, 0), and 3x3 with stride (1, 2), conv output dims even: one launch == conv then the pooling
    kernel bit for bit, within 1e-4 of the oracle, for every implicit-GEMM tile and staging"""
    N, H, W, C, K, k, pad, stride = geo
    case = (N, H, W, C, K, k, pad, stride, (1, 1), 1)
    oh, ow = AU.out_hw(case)
    assert oh % 2 == 0 and ow % 2 == 0 and oh != ow
    d = AU.F32Data(case, seed=AU.seed_of("pool2x2", H), relu=True)
    p = _param(case, d.w, d.b, True)
    want = _nhwc(O.pool_f32_nchw(d.want, (2, 2), (2, 2), (0, 0), 0))
    xd = dev(_nhwc(d.x))
    two = S.SaberConv2D(False).init((N, C, H, W), p, L.F32, L.F32, in_layout=L.NHWC, out_layout=L.NHWC)
    cp = S.SaberConv2DPooling(int8=False).init((N, C, H, W), p, 0, (2, 2), (2, 2), (0, 0), L.F32, L.F32)
    assert cp.fused and cp.out_hw == (oh // 2, ow // 2), (cp.fused, cp.out_hw)
    ran = 0
    for code in [None] + [t | (ks << 8) | (v << 16) for v in (1, 2) for t in range(6) for ks in (1, 4)]:
        if code is not None:
            cp.conv.set_tile(code)
            two.set_tile(code)
        y2 = two.new_output()
        two.dispatch(xd, y2)
        unfused = host(S.pooling_f32(y2, (2, 2), (2, 2), (0, 0), 0, layout=L.NHWC))
        y = cp.new_output()
        y.fill_(float(SENTINEL))
        cp.dispatch(xd, y)
        got = host(y)
        assert cp.algo().endswith("+maxpool2x2"), cp.algo()
        if cp.algo() == two.algo() + "+maxpool2x2":
            assert np.array_equal(got, unfused), cp.algo()
        e_max, e_el = _f32_errors(got, want)
        assert e_max <= FP32_RTOL and e_el <= FP32_RTOL, (cp.algo(), e_max, e_el)
        _reach("conv_f32_pool", cp.algo())
        ran += 1
    assert ran == 25


@pytest.mark.parametrize("name", ["stem_p32", "stem_p23"])
@pytest.mark.parametrize("kind", ["u8", "f32"])
def test_int8_stem_maxpool_with_per_axis_conv_padding(name, kind):
    """SaberConv2DPooling INT8: the 7x7 / 2 stem with pad (3, 2) / (2, 3) + 3x3 / 2 max pooling in one launch == the stem conv then the
    pooling kernel == the oracle's conv then pooling, from a u8 image and from an f32 image quantised on entry"""
    case = CASES[name]
    N, H, W, C, K, k, pad, stride, dil, g = case
    rng = np.random.default_rng(AU.seed_of(name, 40))
    w = (rng.standard_normal((K, 3, 7, 7)) * 0.1).astype(np.float32)
    b = (rng.standard_normal(K) * 0.3).astype(np.float32)
    in_scale, out_scale, odt = 1 / 127.0, 0.02, U8
    if kind == "f32":
        xf = rng.uniform(-1, 1, (N, 3, H, W)).astype(np.float32)
        xq, x_dev, idt, lay = O.quant_nchw_to_nhwc(xf, in_scale, S8), dev(xf), L.F32, L.NCHW
    else:
        xq = AU.rand8(rng, (N, H, W, 3), U8)
        x_dev, idt, lay = dev(xq), U8, L.NHWC
    ws = O.weight_scales(w)
    bp, sc = O.conv_i8_prepare(ws, b, in_scale, out_scale, O.code_of(xq), odt)
    conv_out = O.conv_i8(xq, O.quant_weights(w, ws), bp, sc, odt, 1, pad, stride)
    want = O.pool_i8_nhwc(conv_out, (3, 3), (2, 2), (0, 0), 0)
    p = S.ConvParam(w, b, 1, pad, stride, (1, 1), True)
    cp = S.SaberConv2DPooling().init((N, 3, H, W), p, L.POOL_MAX, (3, 3), (2, 2), (0, 0), idt, odt, in_scale, out_scale, in_layout=lay)
    assert cp.fused and "maxpool" in cp.algo(), cp.algo()
    y = cp.new_output()
    y.fill_(SENTINEL)
    cp.dispatch(x_dev, y)
    got = host(y)
    assert got.shape == want.shape and np.array_equal(got, want), (cp.algo(), _explain(got, want, []))
    conv = S.SaberConv2D(True).init((N, 3, H, W), p, idt, odt, in_scale, out_scale, in_layout=lay)
    assert conv.algo().startswith("stem7x7s2_i8"), conv.algo()
    yc = conv.new_output()
    conv.dispatch(x_dev, yc)
    assert np.array_equal(host(yc), conv_out), conv.algo()
    assert np.array_equal(host(S.pooling_i8(yc, (3, 3), (2, 2), (0, 0), L.POOL_MAX)), got)
    _reach("stem_pool_i8", cp.algo())


# ==== transposition on the device ============================================================================================================
@pytest.mark.parametrize("name", NAMES)
def test_transposed_problem_gives_the_transposed_result(name):
    """conv(x, w; pairs) == transpose of conv(x^T, w^T; every pair swapped), both run on the device with their static selections: a check
    that does not go through the oracle's indexing. Exact for INT8; FP32 within FP32_RTOL (the tap order of the sum changes)."""
    case, tcase = CASES[name], AU.transposed(CASES[name])
    idt, odt, relu = I8_COMBOS[(NAMES.index(name) + 3) % len(I8_COMBOS)]
    d = AU.I8Data(case, idt, odt, relu, True, seed=AU.seed_of(name, 50))
    a = _i8_conv(d)
    t = S.SaberConv2D(True).init((tcase[0], tcase[3], tcase[1], tcase[2]), _param(tcase, np.ascontiguousarray(d.w.transpose(0, 1, 3, 2)), d.b, relu),
                                 idt, odt, d.in_scale, d.out_scale)
    ya, yt = a.new_output(), t.new_output()
    a.dispatch(dev(d.x), ya)
    t.dispatch(dev(d.x.transpose(0, 2, 1, 3)), yt)
    got, got_t = host(ya), host(yt).transpose(0, 2, 1, 3)
    assert got.shape == got_t.shape and np.array_equal(got, got_t), (name, a.algo(), t.algo(), _explain(got_t, got, []))
    f = AU.F32Data(case, seed=AU.seed_of(name, 51))
    N, H, W, C, K = case[:5]
    fa = S.SaberConv2D(False).init((N, C, H, W), _param(case, f.w, f.b, True), L.F32, L.F32, in_layout=L.NHWC, out_layout=L.NHWC)
    ft = S.SaberConv2D(False).init((N, C, W, H), _param(tcase, np.ascontiguousarray(f.w.transpose(0, 1, 3, 2)), f.b, True), L.F32, L.F32,
                                   in_layout=L.NHWC, out_layout=L.NHWC)
    ya, yt = fa.new_output(), ft.new_output()
    fa.dispatch(dev(_nhwc(f.x)), ya)
    ft.dispatch(dev(_nhwc(f.x).transpose(0, 2, 1, 3)), yt)
    e_max, e_el = _f32_errors(host(yt).transpose(0, 2, 1, 3), host(ya))
    assert e_max <= FP32_RTOL and e_el <= FP32_RTOL, (name, fa.algo(), ft.algo(), e_max, e_el)


# ==== pooling ================================================================================================================================
def _same(got, want):
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(got, want, equal_nan=got.dtype == np.float32)


@pytest.mark.parametrize("name", sorted(AU.ASYM_POOL_CASES))
def test_pooling_with_per_axis_windows(name):
    """every pooling kernel over one case: the three types, ceil and floor: S.pooling_i8 (s8, u8), S.pooling_f32 NCHW and NHWC (the vec4
    kernel for C % 4 == 0, the scalar one otherwise), S.pooling_f32_from_i8 and its quantising form - the oracle's bytes (NaN-equal where
    a window is empty); the per-axis output dims agree with the oracle's"""
    case = AU.ASYM_POOL_CASES[name]
    N, H, W, C, win, stride, pad = case
    rng = np.random.default_rng(AU.seed_of(name, 60))
    xs = {S8: AU.rand8(rng, (N, H, W, C), S8), U8: AU.rand8(rng, (N, H, W, C), U8)}
    xf = (rng.standard_normal((N, C, H, W)) * 2.0).astype(np.float32)
    any_pad = pad[0] > 0 or pad[1] > 0
    for floor_mode in (False, True):
        shape = O.pool_out_hw(H, W, pad, win, stride, floor_mode)
        assert shape == AU.pool_out_hw(case, floor_mode)
        assert shape == (S.pool_out_dim(H, pad[0], win[0], stride[0], floor_mode, any_pad), S.pool_out_dim(W, pad[1], win[1], stride[1], floor_mode, any_pad))
        assert shape == S.pool_out_hw(H, W, pad, win, stride, floor_mode)
        for ptype in AU.POOL_TYPES:
            what = (name, ptype, floor_mode)
            for dt, x in xs.items():
                want = O.pool_i8_nhwc(x, win, stride, pad, ptype, floor_mode=floor_mode)
                assert _same(host(S.pooling_i8(dev(x), win, stride, pad, ptype, floor_mode=floor_mode)), want), (what, dt)
                if ptype:      # (max pooling has no f32 output from 8-bit input)
                    want = O.pool_i8_nhwc(x, win, stride, pad, ptype, out_dtype=F32, floor_mode=floor_mode)
                    assert _same(host(S.pooling_i8(dev(x), win, stride, pad, ptype, out_dtype=F32, floor_mode=floor_mode)), want), (what, dt, "f32 out")
                # Pooling<AK_FLOAT> fed the 8-bit tensor: dequantise on entry, f32 NCHW out; and the s8 quantisation of that result
                scale, q_scale = 0.05, 0.07
                wf = O.pool_f32_nchw(O.dequant_nhwc_to_nchw(x, scale), win, stride, pad, ptype, floor_mode=floor_mode)
                assert _same(host(S.pooling_f32_from_i8(dev(x), scale, win, stride, pad, ptype, floor_mode=floor_mode)), wf), (what, dt, "from i8")
                y, yq = S.pooling_f32_from_i8(dev(x), scale, win, stride, pad, ptype, floor_mode=floor_mode, q_scale=q_scale)
                assert _same(host(y), wf) and _same(host(yq), O.quant_flat_s8(wf, q_scale)), (what, dt, "from i8, quantising")
            want = O.pool_f32_nchw(xf, win, stride, pad, ptype, floor_mode=floor_mode)
            assert _same(host(S.pooling_f32(dev(xf), win, stride, pad, ptype, floor_mode=floor_mode)), want), (what, "nchw")
            got = host(S.pooling_f32(dev(_nhwc(xf)), win, stride, pad, ptype, layout=L.NHWC, floor_mode=floor_mode))
            assert _same(got, _nhwc(want)), (what, "nhwc", "vec4" if C % 4 == 0 else "scalar")
    _reach("pool", "c%%4=%d" % (C % 4))


# ==== through the executor ===================================================================================================================
def _inception_block(opt_flags):
    """quantise -> 1x1 -> 1x7 pad (0, 3) -> 7x1 pad (3, 0) -> eltwise sum with the 1x1's output -> 3x2 / (2, 1) max pooling -> global average
    -> fc, at [2, 9, 13, 64]: an Inception-style factorised 7x7. Returns (net, x, oracle edges)."""
    B, H, W, C, NC = 2, 9, 13, 64, 10
    rng = np.random.default_rng(7117)
    x = (rng.standard_normal((B, C, H, W)) * 1.2).astype(np.float32)
    sc = {"data": 0.03, "c1": 0.05, "c17": 0.04, "c71": 0.06, "sum": 0.07}
    geo = {"c1": ((1, 1), (0, 0)), "c17": ((1, 7), (0, 3)), "c71": ((7, 1), (3, 0))}
    src = {"c1": "q", "c17": "c1", "c71": "c17"}
    idt = {"c1": S8, "c17": S8, "c71": U8}
    odt = {"c1": S8, "c17": U8, "c71": S8}
    ref = {"q": O.quant_nchw_to_nhwc(x, sc["data"], S8)}
    sc["q"] = sc["data"]
    net = S.Net()
    net.add_tensor("data", (B, C, H, W), F32)
    net.add_tensor("q", (B, H, W, C), S8)
    net.add_quantize(B, C, H, W, C, S8, sc["data"], "data", "q")
    for nm in ("c1", "c17", "c71"):
        k, pad = geo[nm]
        w = (rng.standard_normal((C, C, k[0], k[1])) * np.sqrt(2.0 / (C * k[0] * k[1]))).astype(np.float32)
        b = (rng.standard_normal(C) * 0.3).astype(np.float32)
        relu = odt[nm] == U8
        ws = O.weight_scales(w)
        bp, s = O.conv_i8_prepare(ws, b, sc[src[nm]], sc[nm], idt[nm], odt[nm])
        ref[nm] = O.conv_i8(ref[src[nm]], O.quant_weights(w, ws), bp, s, odt[nm], relu, pad)
        assert ref[nm].shape == (B, H, W, C)
        conv = S.SaberConv2D(True).init((B, C, H, W), S.ConvParam(w, b, 1, pad, (1, 1), (1, 1), relu), idt[nm], odt[nm], sc[src[nm]], sc[nm])
        net.add_tensor(nm, (B, H, W, C), odt[nm])
        net.add_conv(conv, src[nm], nm)
    c = float(np.float32(1.0 / sc["sum"]))
    ref["sum"] = O.eltwise_i8(ref["c71"], ref["c1"], sc["c71"], sc["c1"], c, c, True)
    net.add_tensor("sum", (B, H, W, C), S8)
    net.add_eltwise_i8(B * H * W * C, sc["c71"], sc["c1"], c, c, True, "c71", "c1", "sum")
    win, st, pd = (3, 2), (2, 1), (0, 0)
    ph, pw = O.pool_out_hw(H, W, pd, win, st)
    assert (ph, pw) == (4, 12) == S.pool_out_hw(H, W, pd, win, st)
    ref["pool"] = O.pool_i8_nhwc(ref["sum"], win, st, pd, 0)
    net.add_tensor("pool", (B, ph, pw, C), S8)
    net.add_pool_i8(B, H, W, C, ph, pw, win, st, pd, 0, S8, S8, "sum", "pool")
    ref["gap"] = O.pool_i8_nhwc(ref["pool"], None, None, None, 1, global_pool=True)
    net.add_tensor("gap", (B, 1, 1, C), S8)
    net.add_pool_i8(B, ph, pw, C, 1, 1, (ph, pw), (ph, pw), (0, 0), 1, S8, S8, "pool", "gap")
    wfc = (rng.standard_normal((NC, C)) * 0.2).astype(np.float32)
    bfc = (rng.standard_normal(NC) * 0.1).astype(np.float32)
    wsf = O.weight_scales(wfc)
    ref["fc"] = O.fc_i8(ref["gap"].reshape(B, C), O.quant_weights(wfc, wsf), wsf, sc["sum"], bfc)
    fc = S.SaberFc(True).init(B, NC, C, wfc, bfc, S8, sc["sum"])
    net.add_tensor("fc", (B, NC), F32)
    net.add_fc(fc, "gap", "fc")
    net.unfused_ops = net.num_ops()
    net.removed = sum(net.optimize(f) for f in opt_flags)
    net.finalize()
    return net, x, ref


@pytest.mark.parametrize("flags", [(), (15,), (15, 16384, 64, 128, 512, 16 | 32 | 256, 4096)], ids=["unfused", "default", "chains_stage_separable"])
def test_inception_style_block_through_the_executor(flags):
    """the op list unfused, with the default optimize flags, and with the chain / stage / separable passes enabled as build_int8_net
    enables them: eager, captured and replayed, and autotuned - every written edge bit-identical to the op-by-op oracle walk; a fusion
    pass either declines or keeps the bytes, and never adds a launch"""
    net, x, ref = _inception_block(flags)
    assert net.unfused_ops == 8
    assert net.num_launches() <= net.unfused_ops
    if not flags:
        assert net.num_launches() == net.unfused_ops and net.removed == 0
    xd = dev(x)

    def compare(what):
        torch.cuda.synchronize()
        checked = []
        for nm in net.tensors:
            if nm == "data" or net.unwritten(nm):
                continue
            got = host(net.tensor(nm))
            assert np.array_equal(got, ref[nm].reshape(got.shape)), (flags, what, nm, _explain(got, ref[nm].reshape(got.shape), []))
            checked.append(nm)
        assert "fc" in checked and "pool" in checked and len(checked) >= (8 if not flags else 5), (flags, what, checked)
        return checked
    net.tensor("data").copy_(xd)
    net.run()
    checked = compare("eager")
    net.tensor("fc").zero_()
    net.capture()
    net.replay()
    compare("replayed")
    net.autotune(iters=2)
    net.tensor("data").copy_(xd)
    net.tensor("fc").zero_()
    net.run()
    compare("autotuned")
    assert net.num_launches() <= net.unfused_ops
    names = [net.op_name(i) for i in range(net.num_ops())]
    for nm in names:
        _reach("net", nm)
    print("flags %s: %d ops, %d launches, edges compared %s; ops: %s" % (flags, net.num_ops(), net.num_launches(), checked, " | ".join(names)))


# ==== guard bands ============================================================================================================================
def _guarded_forms(what, conv, int8, x, out_shape, out_dt, check):
    def launch(T, ws):
        if ws is not None:
            conv.ws = ws
        conv.dispatch(T["x"], T["y"])
    forms = _forms(conv, int8)
    ran = []
    for code, algo in forms:
        conv.set_tile(code)
        got = GU.run_guarded({"x": x}, {"y": (out_shape, out_dt, None)}, launch, "cuda", int(L.load().saber_hip_conv2d_workspace_bytes(conv.h)),
                             plain=TG._plain, what="%s, %s (%s)" % (what, algo, hex(code)))
        torch.cuda.synchronize()
        check(got["y"], algo)
        GU.assert_no_sentinel_run(got["y"], "%s, %s" % (what, algo))
        _reach("guard", algo)
        ran.append(algo)
    _check_against_host(what, conv, ran, int8)
    print("%s: %d guarded forms" % (what, len(forms)))


@pytest.mark.parametrize("name", NAMES)
def test_guard_bands_int8_table(name):
    """every accepted form of every table case once more with every tensor between two 1 MiB guards (tests/guard_util.py): nothing outside
    the tensors is written, the bytes do not depend on the guards' pattern, and they are the oracle's. Per-axis padding is where a read
    outside the image would hide: a kernel that pads the wrong axis reads the neighbouring row - or the guard."""
    case, i = CASES[name], NAMES.index(name)
    idt, odt, relu = I8_COMBOS[(i + 7) % len(I8_COMBOS)]
    d = AU.I8Data(case, idt, odt, relu, True, seed=AU.seed_of(name, 70))
    conv = _i8_conv(d)

    def check(got, algo):
        assert np.array_equal(got, d.want), (name, algo, _explain(got, d.want, _i8_alternatives(d)))
    _guarded_forms("guard i8 %s" % name, conv, True, d.x, d.want.shape, NP_DT[odt], check)


@pytest.mark.parametrize("name", NAMES)
def test_guard_bands_fp32_table(name):
    """the FP32 twin, NHWC (NCHW for C % 4 != 0: the transposing workspace is guarded and dirty): NaN guards, the same bits under both"""
    case = CASES[name]
    N, H, W, C, K, k, pad, stride, dil, g = case
    nchw = C % 4 != 0
    d = AU.F32Data(case, seed=AU.seed_of(name, 71), relu=True)
    lay = L.NCHW if nchw else L.NHWC
    conv = S.SaberConv2D(False).init((N, C, H, W), _param(case, d.w, d.b, True), L.F32, L.F32, in_layout=lay, out_layout=lay)
    want = d.want if nchw else _nhwc(d.want)

    def check(got, algo):
        e_max, e_el = _f32_errors(got, want)
        assert e_max <= FP32_RTOL and e_el <= FP32_RTOL, (name, algo, e_max, e_el)
    _guarded_forms("guard f32 %s" % name, conv, False, d.x if nchw else _nhwc(d.x), want.shape, np.float32, check)


# ==== what ran ===============================================================================================================================
def test_per_axis_cases_reached_every_family():
    """The kernel names the tests above launched cover every family that accepts a per-axis descriptor. (That each test ran exactly the
    forms a descriptor-only handle accepts is asserted where it runs: _check_against_host.) This test reads what the others recorded in
    this process, so it means something only after the whole file ran in file order; under -k, --lf, xdist or a random order it skips."""
    if len(COUNTS) < 6 * len(NAMES) + 40 or not {"pair_i8", "pair_f32", "conv_f32_pool", "stem_pool_i8", "pool", "net"} <= set(REACHED):
        pytest.skip("needs the whole of tests/test_gpu_asym.py run in one process, in file order (%d form runs recorded)" % len(COUNTS))
    r = {k: REACHED.get(k, set()) for k in ("conv_i8", "conv_f32", "fused_i8", "fused_f32", "pair_i8", "pair_f32", "conv_f32_pool", "stem_pool_i8",
                                            "guard", "pool", "net")}
    for fam, names in sorted(r.items()):
        print("%s (%d): %s" % (fam, len(names), " ".join(sorted(names))))
    def conv_families(i8, f32):
        return {
            "igemm_i8 register-staged": [a for a in i8 if a.startswith("igemm_i8_") and not a.startswith("igemm_i8_c4") and "_dma" not in a],
            "igemm_i8 LDS-DMA": [a for a in i8 if a.startswith("igemm_i8_") and a.endswith("_dma")],
            "igemm_i8 wave groups": [a for a in i8 if a.startswith("igemm_i8_") and "_dma_wg" in a],
            "igemm_i8_c4": [a for a in i8 if a.startswith("igemm_i8_c4_")],
            "halo3x3_i8_4x16": [a for a in i8 if a == "halo3x3_i8_4x16"], "halo3x3_i8_8x16": [a for a in i8 if a == "halo3x3_i8_8x16"],
            "image-resident 3x3 (variant 9)": [a for a in i8 if a.startswith("img3x3_i8_")],
            "stem7x7s2_i8": [a for a in i8 if a.startswith("stem7x7s2_i8_")],
            "direct_i8": [a for a in i8 if a == "direct_i8"],
            "igemm_f32 register-staged": [a for a in f32 if a.startswith("igemm_f32_") and "bf16x3" not in a and "_dma" not in a],
            "igemm_f32 LDS-DMA": [a for a in f32 if a.startswith("igemm_f32_") and "bf16x3" not in a and "_dma" in a],
            "bf16-plane tile": [a for a in f32 if a.startswith("igemm_f32_bf16x3_") and "_w8" not in a and "_split" not in a],
            "bf16-plane 8-wave": [a for a in f32 if a.startswith("igemm_f32_bf16x3_") and "_w8" in a],
            "bf16-plane split-K": [a for a in f32 if a.startswith("igemm_f32_bf16x3_") and "_split" in a],
            "direct_f32": [a for a in f32 if a == "direct_f32"],
        }
    want = conv_families(r["conv_i8"], r["conv_f32"])
    want.update({"guarded: " + k: v for k, v in conv_families(r["guard"], r["guard"]).items()})
    want.update({
        "INT8 pair": [a for a in r["pair_i8"] if a.startswith("pair_igemm_i8")], "FP32 pair": [a for a in r["pair_f32"] if a.startswith("pair_igemm_f32")],
        "FP32 conv + max pooling": [a for a in r["conv_f32_pool"] if a.endswith("+maxpool2x2")],
        "INT8 stem + max pooling": [a for a in r["stem_pool_i8"] if "maxpool3x3s2_i8" in a],
        "fused eltwise / sum": r["fused_i8"], "FP32 sum": r["fused_f32"],
        "pooling vec4 and scalar": r["pool"] if r["pool"] >= {"c%4=0", "c%4=2", "c%4=3"} else [],
    })
    print({k: len(v) for k, v in want.items()})
    assert all(want.values()), sorted(k for k, v in want.items() if not v)
    print("%d form runs checked against a descriptor-only enumeration, %d kernel launches' names" % (len(COUNTS), sum(c for _, _, c in COUNTS)))
