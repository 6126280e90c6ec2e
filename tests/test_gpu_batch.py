"""Batch sizes beyond 8 and streaming launches beyond one grid stride, on the GPU (tests/batch_util.py holds the tables; tests/test_batch_cpu.py
checks their preconditions).

A. every launch form - the static selection and every selection code set_tile accepts - at N = 9, 17 (33 for the single convolutions), at
   the smallest spatial sizes, against the oracle over all N images: INT8 bit for bit, FP32 within the two 1e-4 criteria. Composite
   launches go through the routines of their own test modules, which take the batch in their case tuples.
B. every streaming launcher of elementwise.hip with more work items than one grid stride of 8 192 x 256 lanes, against numpy.
C. the executor at batch 9 and 17 (ResNet50 INT8, 224 x 224, default options): every written edge against the library's own batch-8 and
   batch-1 nets on the image slices, and the last image against one oracle walk.
Outputs are poisoned before every launch. The forms that ran are printed per family (pytest -rP shows them)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from anakin_amd import lib as L  # noqa: E402
from anakin_amd import saber as S  # noqa: E402
from anakin_amd import workloads as W  # noqa: E402
from oracle import net_oracle as NO  # noqa: E402
from oracle import oracle as O  # noqa: E402
from tests import batch_util as BU  # noqa: E402
from tests import deconv_util as DU  # noqa: E402
from tests import fire_util as FU  # noqa: E402
from tests import ir_util as IU  # noqa: E402
from tests import sep_util as SU  # noqa: E402
from tests import tail_util as TU  # noqa: E402
from tests import test_gpu_deconv as TD  # noqa: E402
from tests import test_gpu_fire_launch as TF  # noqa: E402
from tests import test_gpu_ir as TI  # noqa: E402
from tests import test_gpu_parity as TP  # noqa: E402
from tests import test_gpu_sep as TS  # noqa: E402
from tests import test_gpu_tail as TT  # noqa: E402

FP32_RTOL = 1e-4      # the project's FP32 contract (tests/test_gpu_resnet.py:_fp32_every_edge)
POISON = 0x5A
# depthwise (16) and grouped (17) selections: the direct kernel (0) and every form number
DW_GROUP_CODES = [(v << 16) | f for v in (16, 17) for f in range(8)]
I8_CODES = TP._I8_CODES + DW_GROUP_CODES
F32_CODES = TP._F32_CODES + DW_GROUP_CODES
CHAIN_CODES = range(16)


@pytest.fixture(scope="module", autouse=True)
def _device():
    L.require_device()  # fail loudly: no fallback path exists


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def fp32_close(got, want, what):
    """the two criteria of _fp32_every_edge: the largest error against the largest value, every element's error against |value| + mean |value|"""
    want = np.asarray(want).reshape(got.shape)
    d = np.abs(got.astype(np.float64) - want)
    e_max = float(d.max() / max(float(np.abs(want).max()), 1e-30))
    e_el = float((d / (np.abs(want) + np.abs(want).mean() + 1e-30)).max())
    assert e_max <= FP32_RTOL and e_el <= FP32_RTOL, (what, e_max, e_el)


# kernel-name fragments that must be among the forms a case ran: a table entry that no longer reaches its kernel family fails here
I8_REACHES = {
    "pw_64_256": ("igemm_i8_", "_dma", "_wg2"),
    "c3x3_64": ("igemm_i8_", "_dma", "halo3x3_i8_4x16", "halo3x3_i8_8x16", "img3x3_i8_1img", "img3x3_i8_2img"),
    "c3x3_64_s2": ("igemm_i8_", "_dma"),
    "pw_64_128_s2": ("igemm_i8_", "_dma"),
    "stem_f32": ("stem7x7s2_i8", "igemm_i8_c4"),
    "stem_s8": ("stem7x7s2_i8", "igemm_i8_c4"),
    "dw_32_s1": ("direct_i8", "dw3x3_i8_px", "dw3x3_i8_rows2"),
    "dw_32_s2": ("direct_i8", "dw3x3_i8_px", "dw3x3_i8_rows2"),
    "g16_64": ("direct_i8", "g3x3_i8_"),
    "g2_64": ("direct_i8", "g3x3_i8_"),
    "c3_5x5": ("igemm_i8_c4",),
    "direct_g2_5x5": ("direct_i8",),
    "pw_elt_pair": ("igemm_i8_", "_dma"),
    "c3x3_32_sum": ("igemm_i8_", "_dma"),
    "pw_sub_res": ("igemm_i8_", "_dma"),
}
F32_REACHES = {
    "c3x3_64": ("igemm_f32_64x64", "igemm_f32_bf16x3_", "_w8", "_split", "halo3x3_f32_bf16x3_"),
    "pw_256_64": ("igemm_f32_64x64", "igemm_f32_bf16x3_", "_w8", "_split", "pw1x1_f32_bf16x3_64ch", "pw1x1_f32_bf16x3_128ch", "pw1x1_f32_bf16x3_ksplit4_"),
    "pw_64_128": ("igemm_f32_bf16x3_", "pw1x1_f32_bf16x3_regs_c64"),
    "dw_32": ("direct_f32", "dw3x3_f32_"),
}


def reaches(tried, fragments, what):
    for f in fragments:
        assert any(f in name for name in tried), (what, "no form named *%s*" % f, sorted(tried))


def every_selection(op, codes, check):
    """check(label) under the static selection and under every code set_tile accepts (one run per kernel name); returns {name: code}"""
    check("static " + op.algo())
    tried = {}
    for code in codes:
        try:
            op.set_tile(code)
        except L.SaberHipError:
            continue
        if op.algo() in tried:
            continue
        tried[op.algo()] = code
        check("%s %s" % (hex(code), op.algo()))
    assert tried
    return tried


def chain_codes(body, case_of, expected):
    """body(case_of(tn)) with the default form (tn = None: no refusal is accepted there) and with every code 0 .. 15; a refused code raises
    at set_tile - the ops themselves were created by the default run already. The accepted set must hold `expected`; beyond it only the
    cooperative forms 7 and 15, which exist together or not at all."""
    body(case_of(None))
    accepted = set()
    for code in CHAIN_CODES:
        try:
            body(case_of(code))
        except L.SaberHipError:
            continue
        accepted.add(code)
    assert accepted - {7, 15} == set(expected) and accepted & {7, 15} in (set(), {7, 15}), (sorted(accepted), sorted(expected))
    return sorted(accepted)


# ==== A: single INT8 convolutions =================================================================================================================
@pytest.mark.parametrize("n", BU.BATCHES)
@pytest.mark.parametrize("name", sorted(BU.I8_CONVS))
def test_int8_conv_every_accepted_selection_is_bit_exact(name, n):
    cs = BU.i8_conv(name, n)
    h, w, c, k, ks, pad, stride, group, idt, odt, relu, kind = cs.geo
    p = S.ConvParam(cs.w, cs.b, group, (pad, pad), (stride, stride), (1, 1), bool(relu))
    if kind == "sum":
        p.res_mode, p.res_relu, p.sum_scale, p.res_dtype = L.RES_SUM_INPLACE, False, BU.I8_SUM_SCALE, odt
    elif kind:
        p.res_mode, p.res_relu, p.sum_scale, p.coeff, p.scale_res = L.RES_ELTWISE, True, 1.0, cs.coeff, BU.I8_RES_SCALE
        if kind == "sub":
            p.res_stride, p.res_hw = 2, cs.res_hw
    conv = S.SaberConv2D(True).init((n, c, h, w), p, idt, odt, cs.in_scale, cs.out_scale, in_layout=L.NCHW if idt == L.F32 else L.NHWC)
    xd = dev(cs.x)
    rd = dev(cs.res) if cs.res is not None else None
    prev = dev(cs.prev) if cs.prev is not None else None

    def check(label):
        y = conv.new_output()
        if prev is not None:
            y.copy_(prev)
        else:
            y.fill_(POISON)
        conv.dispatch(xd, y, rd)
        got = host(y)
        assert got.dtype == cs.want.dtype and got.shape == cs.want.shape, (name, n, label)
        bad = np.nonzero((got != cs.want).reshape(n, -1).any(1))[0]
        assert bad.size == 0, (name, n, label, "images", bad.tolist())
    tried = every_selection(conv, I8_CODES, check)
    reaches(tried, I8_REACHES[name], (name, n))
    print("int8 conv %s N=%d: static + %d forms bit-exact: %s" % (name, n, len(tried), sorted(tried)))


@pytest.mark.parametrize("n", BU.BATCHES)
@pytest.mark.parametrize("kind", ["f32", "s8"])
def test_int8_stem_with_the_fused_max_pooling(kind, n):
    for odt in (O.U8, O.S8):
        TP.test_conv_pooling_stem_fused_vs_oracle((n, 30, 30, 64, kind), odt)


# ==== A: INT8 composites ============================================================================================================================
@pytest.mark.parametrize("n", BU.BATCHES_COMPOSITE)
def test_int8_sibling_pair(n):
    for case in ((n, 7, 9, 64, 256, 64, 1, 0, 1), (n, 9, 7, 128, 128, 48, 1, 0, 2), (n, 6, 6, 32, 128, 16, 3, 1, 1)):
        TP.test_conv_i8_sibling_pair_equals_two_ops(case, O.U8)
    TP.test_conv_i8_sibling_pair_equals_two_ops((n, 7, 9, 64, 256, 64, 1, 0, 1), O.S8)


# the chain-form table of api_chain.hip as tests/test_gpu_parity.py writes it out (the cooperative forms 7 and 15 of the 3x3-led C = 256 chain
# exist together or not at all)
CHAIN_FORMS = {64: {4, 2}, 128: {2, 1, 6, 5}, 256: {1, 9, 11}, 512: {1, 9}}
LED_FORMS = {64: {4, 2}, 128: {2, 1, 6, 5}, 256: {1, 3}}


@pytest.mark.parametrize("n", BU.BATCHES_COMPOSITE)
@pytest.mark.parametrize("c,hw", [(64, 7), (128, 5), (256, 5), (512, 3)])
def test_int8_conv1x1_chain_every_form(c, hw, n):
    got = chain_codes(TP.test_conv1x1_chain_equals_two_launches_and_oracle, lambda tn: (c, n, hw, O.U8, O.U8, 1, 1, tn), CHAIN_FORMS[c])
    print("conv1x1 chain C=%d N=%d: forms %s bit-exact" % (c, n, got))


@pytest.mark.parametrize("n", BU.BATCHES_COMPOSITE)
@pytest.mark.parametrize("c,h,w", [(64, 7, 9), (128, 5, 17), (256, 3, 5)])
def test_int8_conv3x3_led_chain_every_form(c, h, w, n):
    got = chain_codes(TP.test_conv3x3_chain_equals_three_launches_and_oracle, lambda tn: (c, n, h, w, O.U8, O.U8, O.U8, 1, 1, tn), LED_FORMS[c])
    print("conv3x3-led chain C=%d N=%d: forms %s bit-exact" % (c, n, got))


@pytest.mark.parametrize("n", BU.BATCHES_COMPOSITE)
def test_int8_strided_head_chain_with_and_without_the_pair(n):
    got = chain_codes(TP._strided_head, lambda tn: (256, n, 9, 7, O.U8, O.S8, 1, tn), {1, 3})
    got64 = chain_codes(TP._strided_head, lambda tn: (64, n, 9, 11, O.U8, O.U8, 1, tn), {4, 2})
    TP._strided_head_pair((n, 9, 11, O.U8, O.U8, 1, 512, None))      # (None: both forms of its table, 4 and 2)
    TP._strided_head_pair((n, 7, 5, O.S8, O.S8, 0, 128, None))
    print("strided head N=%d: C=256 forms %s, C=64 forms %s, with the pair forms [2, 4] bit-exact" % (n, got, got64))


@pytest.mark.parametrize("n", BU.BATCHES_COMPOSITE)
@pytest.mark.parametrize("kind", ["f32", "s8"])
def test_int8_stem_pair(kind, n):
    TP.test_stem_pool_pair_equals_the_three_ops((n, 30, 30, kind), (O.U8, 256, 64))
    TP.test_stem_pool_pair_equals_the_three_ops((n, 30, 30, kind), (O.S8, 64, 256))


@pytest.mark.parametrize("n", BU.BATCHES_COMPOSITE)
def test_int8_separable_launch_five_forms(n):
    """K = 320 > 256: both K-splitting widths have two slices, so all five forms of conv_sep.hip exist"""
    codes = TS.run_case(SU.Case((n, 32, 9, 7, 1, 1, 320), SU.DTYPES[0], SU.BIASES[0], 20290 + n))
    assert codes == [1, 2, 3, 4, 5], codes
    codes2 = TS.run_case(SU.Case((n, 64, 11, 13, 2, 1, 128), SU.DTYPES[2], SU.BIASES[1], 20291 + n))
    assert codes2 == [1, 2, 5], codes2
    print("separable N=%d: forms %s and %s bit-exact on both edges" % (n, codes, codes2))


@pytest.mark.parametrize("n", BU.BATCHES_COMPOSITE)
def test_int8_inverted_residual_launch_three_forms(n):
    codes = TI.run_case(IU.Case((16, 96, 16, 5, 7, 1, True, n), (IU.S8, True, 0, 1), IU.BIASES[0], 20292 + n))
    assert codes == [1, 2, 3], codes
    codes2 = TI.run_case(IU.Case((24, 144, 32, 9, 11, 2, False, n), (IU.U8, False, 1, 0), IU.BIASES[1], 20293 + n))
    assert codes2 == [1, 2, 3], codes2
    print("inverted residual N=%d: forms %s and %s bit-exact on every edge" % (n, codes, codes2))


@pytest.mark.parametrize("n", BU.BATCHES_COMPOSITE)
def test_int8_fire_launch_two_forms(n):
    for geo, seed in (((16, 16, 16, 16, 5, 7, n), 20294), ((64, 16, 48, 80, 9, 17, n), 20295)):
        assert TF.run_case(FU.FireCase(geo, FU.U8, FU.BIASES[0], seed + n)) == [1, 2]
    print("fire N=%d: forms [1, 2] bit-exact on both edges, two geometries" % n)


@pytest.mark.parametrize("n", BU.BATCHES_COMPOSITE)
@pytest.mark.parametrize("epi", [TU.GPOOL_EPILOGUES[0], TU.GPOOL_EPILOGUES[2]], ids=lambda e: e[0])
def test_int8_conv_eltwise_global_pooling(epi, n):
    TT.test_conv1x1_with_global_pooling_equals_oracle(7, 7, n, 2048, epi)


@pytest.mark.parametrize("m", BU.FC_ROWS)
def test_int8_fc_and_softmax(m):
    """logits bit for bit under every accepted selection; prob = softmax of the logits within the existing criterion, through the one
    entry point; beyond 16 rows the small-batch kernel (and with it the one-launch form) is refused"""
    cs = BU.fc_case(m)
    small = m <= BU.FC_SMALL_MAX_ROWS
    for dt in (L.S8, L.U8):
        fc = S.SaberFc(True).init(m, BU.FC_N, BU.FC_K, cs.wq, cs.b, dt, BU.FC_IN_SCALE, 0.5 if dt == L.U8 else 1.0, w_scale=cs.ws)
        assert (fc.algo() == "fc_i8_small_16xk4") == small, (m, fc.algo())
        xd, want = dev(cs.x[dt]), cs.want[dt]
        sm = O.softmax_f32(want)
        y = torch.empty((m, BU.FC_N), dtype=torch.float32, device="cuda")
        p = torch.empty_like(y)

        def check_prob(label):
            y.fill_(7.0)
            p.fill_(-1.0)
            fc.dispatch_softmax(xd, y, p)
            got_y, got_p = host(y), host(p)
            assert np.array_equal(got_y, want), (m, dt, label)
            assert np.abs(got_p - sm).max() <= FP32_RTOL * sm.max() and np.allclose(got_p.sum(1), 1.0, atol=1e-5), (m, dt, label)
            two = host(S.softmax(y))
            assert np.abs(got_p - two).max() <= FP32_RTOL * two.max(), (m, dt, label)
        check_prob("static " + fc.algo())
        if not small:
            with pytest.raises(L.SaberHipError):
                fc.set_tile(10 << 16)
            check_prob("after the refusal " + fc.algo())

        def check(label):
            y.fill_(7.0)
            assert np.array_equal(host(fc.dispatch(xd, y)), want), (m, dt, label)
        tried = every_selection(fc, TP._I8_CODES + [10 << 16], check)
        assert ("fc_i8_small_16xk4" in tried) == small, sorted(tried)
        print("int8 fc m=%d dtype %d: %d forms bit-exact: %s" % (m, dt, len(tried), sorted(tried)))


# ==== A: FP32 ==========================================================================================================================================
@pytest.mark.parametrize("n", BU.BATCHES_COMPOSITE)
@pytest.mark.parametrize("name", sorted(BU.F32_CONVS))
def test_fp32_conv_every_accepted_selection_within_tolerance(name, n):
    cs = BU.f32_conv(name, n)
    h, w, c, k, ks, pad, group = cs.geo
    p = S.ConvParam(cs.w, cs.b, group, (pad, pad), (1, 1), (1, 1), True)
    conv = S.SaberConv2D(False).init((n, c, h, w), p, L.F32, L.F32, in_layout=L.NHWC, out_layout=L.NHWC)
    xd = dev(cs.x.transpose(0, 2, 3, 1))

    def check(label):
        y = conv.new_output()
        y.fill_(float("nan"))
        conv.dispatch(xd, y)
        got = host(y).transpose(0, 3, 1, 2)
        fp32_close(got, cs.want, (name, n, label))
        y2 = conv.new_output()
        y2.fill_(float("nan"))
        conv.dispatch(xd, y2)
        assert np.array_equal(host(y2).transpose(0, 3, 1, 2), got), ("not deterministic", name, n, label)
    tried = every_selection(conv, F32_CODES, check)
    reaches(tried, F32_REACHES[name], (name, n))
    print("fp32 conv %s N=%d: static + %d forms within 1e-4: %s" % (name, n, len(tried), sorted(tried)))


@pytest.mark.parametrize("n", BU.BATCHES_COMPOSITE)
def test_fp32_sibling_pair_and_conv_relu_pooling(n):
    TP.test_conv_f32_sibling_pair_equals_two_ops((n, 9, 7, 128, 128, 48, 1, 0, 2))
    TP.test_conv_f32_sibling_pair_equals_two_ops((n, 6, 6, 32, 128, 16, 3, 1, 1))
    TP.test_conv_f32_fused_relu_maxpool2x2((n, 16, 8, 8, 32, 3, 1))
    TP.test_conv_f32_fused_relu_maxpool2x2((n, 8, 6, 10, 20, 1, 0))


@pytest.mark.parametrize("variant", [0, 1, 2, 3])
def test_fp32_stem_one_launch_at_batch_17(variant):
    TP.test_stem_f32_one_launch_vs_oracle_and_the_three_ops((17, 64, 64), variant)


@pytest.mark.parametrize("n", BU.BATCHES_COMPOSITE)
@pytest.mark.parametrize("ks,pad", [(2, 0), (4, 1)])
def test_fp32_deconv_three_forms(ks, pad, n):
    cs = DU.case(n, 5, 6, 32, 16, ks, pad=(pad, pad))
    x, w, b = DU.make(cs, np.random.default_rng([20296, ks, n]))
    want = DU.deconv_ref(x, w, b, cs, True)
    assert BU.distinct_images(want)
    op = TD._op(cs, w, b, True)
    assert op.forms() == [0, 1, 2], op.forms()
    for f in op.forms():
        DU.fp32_close(TD._run(op, x, f), want, ("deconv k%d" % ks, n, TD.NAMES[f]))


@pytest.mark.parametrize("m", BU.FC_F32_ROWS)
def test_fp32_fc_beyond_the_small_batch_kernel(m):
    cs = BU.fc_case(m)
    xd = dev(cs.xf)
    for kn in (False, True):
        fc = S.SaberFc(False).init(m, BU.FC_N, BU.FC_K, np.ascontiguousarray(cs.w.T) if kn else cs.w, cs.b, L.F32, w_is_kn=kn)
        assert not fc.algo().startswith("fc_f32_small"), fc.algo()
        y = torch.empty((m, BU.FC_N), dtype=torch.float32, device="cuda")

        def check(label):
            y.fill_(float("nan"))
            fp32_close(host(fc.dispatch(xd, y)), cs.want_f32, (m, kn, label))
        tried = every_selection(fc, TP._F32_CODES, check)
        assert not any(a.startswith("fc_f32_small") for a in tried), sorted(tried)
        print("fp32 fc m=%d w_is_kn=%s: %d forms within 1e-4: %s" % (m, kn, len(tried), sorted(tried)))


def test_fp32_gemm_trans_b_beyond_the_row_kernel():
    """Gemm with trans_b at m = 17 (gemm_f32_rows takes m <= 16) and at 16 beside it"""
    cs = BU.fc_case(17)
    for m in (BU.GEMM_ROWS, 16):
        a = cs.xf[:m]
        want = O.gemm_f32(a, cs.w, m, BU.FC_N, BU.FC_K, False, True, 1.0, 0.0)
        c = torch.full((m, BU.FC_N), float("nan"), dtype=torch.float32, device="cuda")
        fp32_close(host(S.gemm(False, True, m, BU.FC_N, BU.FC_K, 1.0, dev(a), dev(cs.w), 0.0, c)), want, ("gemm trans_b", m))


# ==== A: pooling over batch =========================================================================================================================
@pytest.mark.parametrize("n", BU.GPOOL_BATCHES)
@pytest.mark.parametrize("dt", [O.S8, O.U8])
def test_int8_global_average_pooling_across_the_grid_y_limit(dt, n):
    x = BU.gpool_input(n, dt)
    xd = dev(x)
    for od, fill in ((None, POISON), (L.F32, float("nan"))):
        want = O.pool_i8_nhwc(x, None, None, None, 1, out_dtype=None if od is None else O.F32, global_pool=True)
        out = torch.empty(want.shape, dtype=S._TORCH_DT[O.code_of(want)], device="cuda")
        out.fill_(fill)
        got = host(S.pooling_i8(xd, None, None, None, 1, out_dtype=od, global_pooling=True, out=out))
        bad = np.nonzero((got != want).reshape(n, -1).any(1))[0]
        assert bad.size == 0, (n, dt, od, "images", bad[:8].tolist(), bad.size)


@pytest.mark.parametrize("i", range(len(BU.POOL_CASES)))
def test_pooling_kernels_at_batch_17(i):
    win, st, pad, pt, c = BU.POOL_CASES[i]
    for dt in (O.S8, O.U8):
        x = BU.pool_input(i, dt)
        want = O.pool_i8_nhwc(x, win, st, pad, pt)
        out = torch.full(want.shape, POISON, dtype=S._TORCH_DT[dt], device="cuda")
        assert np.array_equal(host(S.pooling_i8(dev(x), win, st, pad, pt, out=out)), want), (i, dt)
        wq = O.pool_f32_nchw(O.dequant_nhwc_to_nchw(x, 0.043), win, st, pad, pt)
        out = torch.full(wq.shape, float("nan"), dtype=torch.float32, device="cuda")
        assert np.array_equal(host(S.pooling_f32_from_i8(dev(x), 0.043, win, st, pad, pt, out=out)), wq), (i, dt, "f32 from 8-bit")
    xh = BU.pool_input(i, O.F32)
    xc = np.ascontiguousarray(xh.transpose(0, 3, 1, 2))
    want = O.pool_f32_nchw(xc, win, st, pad, pt)
    out = torch.full(want.shape, float("nan"), dtype=torch.float32, device="cuda")
    assert np.array_equal(host(S.pooling_f32(dev(xc), win, st, pad, pt, out=out)), want), (i, "nchw")
    out = torch.full(want.transpose(0, 2, 3, 1).shape, float("nan"), dtype=torch.float32, device="cuda")
    assert np.array_equal(host(S.pooling_f32(dev(xh), win, st, pad, pt, layout=L.NHWC, out=out)), want.transpose(0, 2, 3, 1)), (i, "nhwc")


# ==== B: streaming launchers on their second grid-stride trip ===================================================================================
def _launch_stream_case(cs, T):
    """one launch of the case on the device tensors T (inputs by name, "y": the poisoned output)"""
    la = cs["launcher"]
    win = ((2, 2), (1, 1), (0, 0))
    if la == "launch_quantize_nchw_to_nhwc":
        return S.quantize_nchw_to_nhwc(T["x"], cs["scale"], cs["odt"], c_pad=cs["c_pad"], out=T["y"])
    if la == "launch_dequantize_nhwc_to_nchw":
        return S.dequantize_nhwc_to_nchw(T["x"], cs["scale"], out=T["y"])
    if la == "launch_transpose_nchw_to_nhwc_f32":
        return S.transpose_nchw_to_nhwc(T["x"], cs["c_pad"], out=T["y"])
    if la == "launch_transpose_nhwc_to_nchw_f32":
        return S.transpose_nhwc_to_nchw(T["x"], cs["c"], out=T["y"])
    if la == "launch_quantize_flat_s8":
        return S.quantize_flat_s8(T["x"], cs["scale"], out=T["y"])
    if la == "launch_eltwise_sum_i8":
        return S.eltwise_sum(T["a"], T["b"], (cs["c0"], cs["c1"]), cs["relu"], cs["sa"], cs["sb"], out=T["y"])
    if la == "launch_eltwise_sum_f32":
        return S.eltwise_sum(T["a"], T["b"], (cs["c0"], cs["c1"]), cs["relu"], out=T["y"])
    if la == "launch_relu_f32":
        return S.activation(S.ACTIVE_RELU, T["x"], T["y"])
    if la == "launch_activation_f32":
        return S.activation(S.ACTIVE_CLIPPED_RELU, T["x"], T["y"], 0.0, cs["coef"])
    if la == "launch_prelu_f32":
        return S.prelu(T["x"], T["slope"], cs["shape"][1], cs["shape"][2], False, T["y"])
    if la == "launch_concat_nhwc":
        return S.SaberConcat().init(cs["channels"], L.S8).dispatch([T["x%d" % i] for i in range(len(cs["channels"]))], out=T["y"])
    if la == "launch_pool2d_i8_nhwc":
        return S.pooling_i8(T["x"], *win, cs["ptype"], out=T["y"])
    if la == "launch_pool2d_f32":
        return S.pooling_f32(T["x"], *win, 0, layout=L.NCHW if cs["layout"] == "nchw" else L.NHWC, out=T["y"])
    if la == "launch_pool2d_f32_from_i8":
        return S.pooling_f32_from_i8(T["x"], cs["scale"], *win, 0, out=T["y"])
    raise KeyError(la)


@pytest.mark.parametrize("name", sorted(BU.STREAM_CASES))
def test_streaming_launcher_beyond_one_grid_stride(name):
    cs = BU.STREAM_CASES[name]
    arrays = BU.stream_inputs(name)
    want = BU.stream_reference(name, arrays)
    T = {k: dev(v) for k, v in arrays.items()}
    T["y"] = torch.empty(want.shape, dtype={np.float32: torch.float32, np.int8: torch.int8, np.uint8: torch.uint8}[want.dtype.type], device="cuda")
    if want.dtype == np.float32:
        T["y"].fill_(float("nan"))
    else:
        T["y"].fill_(POISON)
    got = host(_launch_stream_case(cs, T))
    del T
    assert got.shape == want.shape and got.dtype == want.dtype, (name, got.shape, want.shape)
    bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
    assert bad.size == 0, (name, cs["items"], "first / last / count of wrong flat indices", int(bad[0]), int(bad[-1]), int(bad.size))
    torch.cuda.empty_cache()


def test_pad_channels_beyond_one_grid_stride():
    """pad_channels_i8 is internal to the C = 3 implicit-GEMM stem path (selection 8 << 16): one 725 x 725 u8 image pads 2 102 500 bytes;
    a 3x3 conv to 8 channels keeps the oracle under a second"""
    n, h, w, c = BU.PAD_CHANNELS_CASE["shape"]
    k = BU.PAD_CHANNELS_CASE["k"]
    rng = np.random.default_rng(20297)
    x = BU.rand8(rng, (n, h, w, c), O.U8)
    wt = (rng.standard_normal((k, c, 3, 3)) * 0.3).astype(np.float32)
    b = (rng.standard_normal(k) * 0.5).astype(np.float32)
    ws = O.weight_scales(wt)
    bp, sc = O.conv_i8_prepare(ws, b, 0.02, 0.05, O.U8, O.S8)
    want = O.conv_i8(x, O.quant_weights(wt, ws), bp, sc, O.S8, 0, (1, 1))
    conv = S.SaberConv2D(True).init((n, c, h, w), S.ConvParam(wt, b, 1, (1, 1), (1, 1), (1, 1), False), L.U8, L.S8, 0.02, 0.05)
    conv.set_tile(8 << 16)
    assert conv.algo().startswith("igemm_i8_c4"), conv.algo()
    y = conv.new_output()
    y.fill_(POISON)
    conv.dispatch(dev(x), y)
    got = host(y)
    bad = np.flatnonzero((got != want).reshape(-1, k).any(1))
    assert bad.size == 0, ("output pixels", int(bad[0]), int(bad[-1]), int(bad.size))
    torch.cuda.empty_cache()


# ==== C: the executor at batch 9 and 17 =============================================================================================================
def _poison_run_read(net, x):
    """one pass on x with every written edge poisoned first: {name: array} of the edges the pass writes under the current selection (an
    edge the optimiser removed has no storage, one that stays in LDS is not written: Net.unwritten names both) - each of them must
    have lost its poison"""
    live = [name for name in net.tensors if name != "data" and not net.unwritten(name)]
    for name in live:
        net.tensor(name).view(torch.uint8).fill_(POISON)
    net.tensor("data").copy_(torch.from_numpy(x).cuda())
    net.run()
    torch.cuda.synchronize()
    out = {}
    for name in live:
        t = net.tensor(name)
        assert bool((t.view(torch.uint8) != POISON).any().item()), (name, "declared written, still poison after the pass")
        out[name] = t.cpu().numpy()
    return out


@pytest.fixture(scope="module")
def resnet():
    """the model, 17 images, scales calibrated on the first two, and the library's own batch-8 and batch-1 nets (pinned to the oracle by
    tests/test_gpu_resnet.py) run on the slices [0:8], [8:16], [8:9], [16:17]: computed once, never modified"""
    model = W.build_model("resnet50")
    x = W.make_input(17)
    scales = W.calibrate(model, x[:2])
    net8 = W.build_int8_net(model, dict(scales), 8)
    net1 = W.build_int8_net(model, dict(scales), 1)
    assert any(sel for _, _, sel in net8.stages())      # (the batch-8 net does run its stage launch: the large nets must not)
    small = {(0, 8): _poison_run_read(net8, x[0:8]), (8, 16): _poison_run_read(net8, x[8:16]),
             (8, 9): _poison_run_read(net1, x[8:9]), (16, 17): _poison_run_read(net1, x[16:17])}
    del net8, net1
    torch.cuda.empty_cache()
    return model, x, scales, small


def _same_edge(name, got, want, what):
    """tests/test_gpu_resnet.py's rule: prob within 1e-4 of its largest value, every other edge - the logits too - exactly"""
    want = want.reshape(got.shape)
    if name == "prob":
        assert np.abs(got - want).max() <= 1e-4 * want.max(), what
    else:
        assert np.array_equal(got, want), what


@pytest.mark.parametrize("n", BU.BATCHES_COMPOSITE)
def test_resnet50_int8_executor_beyond_batch_8(resnet, n):
    model, x17, scales, small = resnet
    x = x17[:n]
    net = W.build_int8_net(model, dict(scales), n)
    # no stage launch (it holds an image per XCD: batch <= 8), so the launches are the chain-only configuration's; fc + softmax are one
    # launch up to 16 rows and two beyond
    assert not [s for s in net.stages() if s[2]], net.stages()
    assert net.fc_softmaxed == (1 if n <= BU.FC_SMALL_MAX_ROWS else 0)
    chain_only = W.build_int8_net(model, dict(scales), n, stage=False)
    assert net.num_launches() == chain_only.num_launches(), (net.num_launches(), chain_only.num_launches())
    if n > BU.FC_SMALL_MAX_ROWS:
        assert net.num_launches() == W.build_int8_net(model, dict(scales), n, stage=False, fc_softmax=False).num_launches()
    del chain_only
    big = _poison_run_read(net, x)
    assert "fc1000" in big and "prob" in big
    # 1. the library's own batch-8 / batch-1 nets on the slices: every edge written by both, image by image
    slices = [(0, 8), (8, 9)] if n == 9 else [(0, 8), (8, 16), (16, 17)]
    for lo, hi in slices:
        both = [nm for nm in big if nm in small[lo, hi]]
        assert len(both) >= 39 and "fc1000" in both and "prob" in both, (lo, hi, len(both))
        for nm in both:
            _same_edge(nm, big[nm][lo:hi], small[lo, hi][nm], (n, "images %d:%d" % (lo, hi), nm))
    # 2. the last image against the oracle's own walk
    ref = NO.run_int8(model, dict(scales), x[n - 1:n])
    checked = 0
    for nm, got in big.items():
        if nm in ref:
            _same_edge(nm, got[n - 1:n], ref[nm], (n, "last image against the oracle", nm))
            checked += 1
    assert checked >= 39, checked
    print("ResNet50 INT8 batch %d: %d launches, %d written edges, %d of them equal to the oracle on the last image" % (n, net.num_launches(), len(big), checked))
    # hipGraph replay, the autotuned selection and the compacted arena reproduce the eager pass
    logits, prob = big["fc1000"], big["prob"]
    net.tensor("fc1000").zero_()
    net.capture()
    net.replay()
    assert np.array_equal(host(net.tensor("fc1000")), logits)
    net.autotune(iters=2)
    net.tensor("data").copy_(torch.from_numpy(x).cuda())
    net.tensor("fc1000").zero_()
    net.run()
    assert np.array_equal(host(net.tensor("fc1000")), logits)
    tuned = host(net.tensor("prob")).copy()      # (the tuner may have chosen the other fc + softmax form: the same logits, prob within the criterion)
    assert np.abs(tuned - prob).max() <= 1e-4 * prob.max()
    net.compact()
    assert net.compacted()
    net.tensor("data").copy_(torch.from_numpy(x).cuda())
    net.tensor("prob").zero_()
    net.run()
    assert np.array_equal(host(net.tensor("fc1000")), logits) and np.array_equal(host(net.tensor("prob")), tuned)
