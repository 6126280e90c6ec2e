"""Per-axis geometry on the host (no GPU): the oracle is pinned to the reference and to plain numpy at kh != kw, pad_h != pad_w,
stride_h != stride_w and dil_h != dil_w; the shared case table (tests/asym_util.py) can see every axis swap; and create() / set_tile()
accept and refuse the per-axis descriptors family by family as the kernels' rules say. tests/test_gpu_asym.py runs the same cases on the
device."""
import numpy as np
import pytest

from anakin_amd import build as B
from anakin_amd import lib as L
from oracle import oracle as O
from tests import asym_util as AU

import os

F32, S8, U8 = O.F32, O.S8, O.U8
CASES = AU.ASYM_CONV_CASES
NAMES = sorted(CASES)
POOLS = AU.ASYM_POOL_CASES
needs_ref = pytest.mark.skipif(not O.ref_available(), reason="oracle/_ref not built")
FP32_RTOL = 1e-4      # the project's FP32 tolerance (tests/test_gpu_parity.py)


def _f32_criteria(got, want):
    d = np.abs(got.astype(np.float64) - want.astype(np.float64))
    return d.max() / np.abs(want).max(), (d / (np.abs(want) + np.abs(want).mean())).max()


# ---- an independent convolution: float64 numpy, one strided slice per tap ----------------------------------------------------------------
def np_conv_nhwc(x, w, pad, stride, dil, group):
    """x [N, H, W, C], w [K, C / group, kh, kw] -> float64 [N, oh, ow, K]; the H axis uses index 0 of every pair, the W axis index 1"""
    N, H, W, C = x.shape
    K, Cg, kh, kw = w.shape
    Kg = K // group
    oh = (H + 2 * pad[0] - dil[0] * (kh - 1) - 1) // stride[0] + 1
    ow = (W + 2 * pad[1] - dil[1] * (kw - 1) - 1) // stride[1] + 1
    xp = np.zeros((N, H + 2 * pad[0], W + 2 * pad[1], C), np.float64)
    xp[:, pad[0]:pad[0] + H, pad[1]:pad[1] + W, :] = x
    wg = w.astype(np.float64).reshape(group, Kg, Cg, kh, kw)
    out = np.zeros((N, oh, ow, group, Kg), np.float64)
    for i in range(kh):
        r0 = i * dil[0]
        for j in range(kw):
            c0 = j * dil[1]
            patch = xp[:, r0:r0 + (oh - 1) * stride[0] + 1:stride[0], c0:c0 + (ow - 1) * stride[1] + 1:stride[1], :]
            out += np.einsum("nhwgc,gkc->nhwgk", patch.reshape(N, oh, ow, group, Cg), wg[:, :, :, i, j])
    return out.reshape(N, oh, ow, K)


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("idt", [S8, U8])
def test_int8_accumulators_equal_a_numpy_convolution(name, idt):
    case = CASES[name]
    d = AU.I8Data(case, idt, S8, 0, seed=AU.seed_of(name, idt))
    acc = O.conv_i8_acc(d.x, d.wq, case[6], case[7], case[8], case[9])
    want = np_conv_nhwc(d.x.astype(np.float64), d.wq, case[6], case[7], case[8], case[9])
    assert acc.shape == want.shape == (case[0],) + AU.out_hw(case) + (case[4],)
    assert np.array_equal(acc.astype(np.float64), want)      # (integers below 2^31: exact in float64)
    assert len(np.unique(acc)) > 50


@pytest.mark.parametrize("name", NAMES)
def test_fp32_oracle_equals_a_numpy_convolution(name):
    case = CASES[name]
    d = AU.F32Data(case, seed=AU.seed_of(name), relu=False)
    want = np_conv_nhwc(d.x.transpose(0, 2, 3, 1), d.w, case[6], case[7], case[8], case[9]) + d.b.astype(np.float64)
    got = d.want.transpose(0, 2, 3, 1)
    assert got.shape == want.shape
    assert np.abs(got - want).max() <= 1e-5 * np.abs(want).max()


# ---- oracle against the compiled reference ------------------------------------------------------------------------------------------------
@needs_ref
@pytest.mark.parametrize("name", NAMES)
def test_int8_oracle_equals_the_reference(name):
    """O.conv_i8 == the reference's INT8 convolution bit for bit, fed the f32 weights (it quantises them) and fed s8 weights with scales;
    s8 / u8 input x s8 / u8 + relu / f32 output"""
    case = CASES[name]
    for idt in (S8, U8):
        for odt, relu in ((S8, 0), (S8, 1), (U8, 1), (F32, 0), (F32, 1)):
            d = AU.I8Data(case, idt, odt, relu, seed=AU.seed_of(name, idt))
            # an in-range output scale, from the oracle's own f32 result: the reference's GEMM path casts without saturating, which the
            # project documents as undefined and does not follow
            d.out_scale = float(np.abs(d.oracle(odt=F32)).max()) / (120.0 if odt != U8 else 240.0 * 127 / 255)
            geo = (case[6], case[7], case[8], case[9])
            a = O.ref_conv_i8(d.x, d.w, None, d.b, d.in_scale, d.out_scale, odt, relu, *geo)
            b = O.ref_conv_i8(d.x, d.wq, d.ws, d.b, d.in_scale, d.out_scale, odt, relu, *geo)
            assert d.want.shape == a.shape and np.array_equal(d.want, a), (name, idt, odt, relu, "f32 weights")
            assert np.array_equal(d.want, b), (name, idt, odt, relu, "s8 weights")
            assert len(np.unique(d.want)) > 20


@needs_ref
@pytest.mark.parametrize("name", NAMES)
def test_fp32_oracle_equals_the_reference(name):
    """O.conv_f32_nchw == conv_basic_check bit for bit; on one group also within 1e-4 (both criteria) of the production x86 convolution"""
    case = CASES[name]
    for relu in (False, True):
        d = AU.F32Data(case, seed=AU.seed_of(name, int(relu)), relu=relu)
        geo = (case[6], case[7], case[8], case[9])
        assert np.array_equal(d.want, O.ref_conv_basic_check_f32(d.x, d.w, d.b, relu, *geo)), (name, relu)
        if case[9] == 1:
            prod, used = O.ref_conv_f32(d.x, d.w, d.b, relu, *geo)
            e_max, e_el = _f32_criteria(d.want, prod)
            assert e_max <= FP32_RTOL and e_el <= FP32_RTOL, (name, relu, O.REF_F32_IMPL_NAME.get(used, used), e_max, e_el)


# ---- the cases can see a swap -------------------------------------------------------------------------------------------------------------
def _visible(true, other, what):
    if other is None or other.shape != true.shape:
        return
    frac = float(np.mean(true != other))
    assert frac >= 0.01, "%s: only %.3f %% of the outputs change" % (what, 100 * frac)


@pytest.mark.parametrize("name", NAMES)
def test_every_axis_swap_changes_the_output(name):
    """A condition on the inputs: for every pair of the case that differs, the oracle's output with that pair swapped, with either
    axis's value used for both, or with the taps transposed, has another shape or differs in at least 1 % of its elements - INT8 bytes
    of both input types and FP32 values. A device kernel with such a defect cannot equal the oracle on this case."""
    case = CASES[name]
    sits = AU.swap_situations(case)
    assert sits
    for idt in (S8, U8):
        d = AU.I8Data(case, idt, S8, 0, seed=AU.seed_of(name, idt))
        for label, how, pad, stride, dil in sits:
            if AU.situation_out_hw(case, how, pad, stride, dil) is None:
                continue
            other = d.oracle(wq=AU.swapped_weights(d.wq, how), pad=pad, stride=stride, dil=dil)
            _visible(d.want, other, "%s, %s, input %d" % (name, label, idt))
    f = AU.F32Data(case, seed=AU.seed_of(name))
    for label, how, pad, stride, dil in sits:
        if AU.situation_out_hw(case, how, pad, stride, dil) is None:
            continue
        _visible(f.want, f.oracle(w=AU.swapped_weights(f.w, how), pad=pad, stride=stride, dil=dil), "%s, %s, f32" % (name, label))


@pytest.mark.parametrize("name", NAMES)
def test_transposition_identity_on_the_oracle(name):
    """conv(x, w; pairs) == the H <-> W transpose of conv(x^T, w^T; every pair swapped): exact for INT8 (integer accumulation, the same
    float32 epilogue per element), within 1e-4 for FP32 (the tap order of the sum changes)"""
    case, tcase = CASES[name], AU.transposed(CASES[name])
    for idt, odt, relu in ((S8, S8, 0), (U8, U8, 1), (U8, F32, 0)):
        d = AU.I8Data(case, idt, odt, relu, seed=AU.seed_of(name, idt))
        t = O.conv_i8(d.x.transpose(0, 2, 1, 3), d.wq.transpose(0, 1, 3, 2), *O.conv_i8_prepare(d.ws, d.b, d.in_scale, d.out_scale, idt, odt),
                      odt, relu, tcase[6], tcase[7], tcase[8], group=tcase[9])
        assert np.array_equal(t.transpose(0, 2, 1, 3), d.want), (name, idt, odt)
    f = AU.F32Data(case, seed=AU.seed_of(name))
    t = O.conv_f32_nchw(f.x.transpose(0, 1, 3, 2), f.w.transpose(0, 1, 3, 2), f.b, True, tcase[6], tcase[7], tcase[8], group=tcase[9])
    e_max, e_el = _f32_criteria(t.transpose(0, 1, 3, 2), f.want)
    assert e_max <= FP32_RTOL and e_el <= FP32_RTOL, (name, e_max, e_el)


def test_random_asym_geometry_draws():
    """the generator: reproducible, never an empty output, always a pair that differs, and over 200 draws every pair differs somewhere"""
    seen = set()
    for int8 in (True, False):
        for seed in range(100):
            a = AU.random_asym_geometry(np.random.default_rng(seed), int8)
            assert a == AU.random_asym_geometry(np.random.default_rng(seed), int8)
            N, H, W, C, K, k, pad, stride, dil, g = a
            assert min(AU.out_hw(a)) >= 1 and AU.differing_pairs(a) and g == 1
            assert all(v in (1, 3, 5, 7) for v in k) and all(v in (1, 2) for v in stride + dil)
            assert all(dil[i] == 1 for i in range(2) if k[i] == 1)
            assert all(pad[i] in (0, 1, dil[i] * (k[i] - 1) // 2) for i in range(2))
            seen |= set(AU.differing_pairs(a))
    assert seen == set(AU.PAIRS)


# ---- pooling ------------------------------------------------------------------------------------------------------------------------------
def test_pool_table_covers_what_it_names():
    wins = {c[4] for c in POOLS.values()}
    strides = {c[5] for c in POOLS.values()}
    pads = {c[6] for c in POOLS.values()}
    assert {(2, 3), (3, 2), (1, 3), (5, 2)} <= wins and {(2, 1), (1, 2), (3, 1)} <= strides and {(0, 1), (1, 0), (2, 0)} <= pads
    assert {c[3] for c in POOLS.values()} >= {3, 10, 16, 64}
    for name, (N, H, W, C, win, stride, pad) in POOLS.items():
        assert H != W and pad[0] < win[0] and pad[1] < win[1], name
    # a ceil-mode window hangs over the far edge of ONE axis only, with and without padding on that axis
    over = []
    for name, c in POOLS.items():
        N, H, W, C, win, stride, pad = c
        oh, ow = AU.pool_out_hw(c, False)
        over.append(((oh - 1) * stride[0] - pad[0] + win[0] > H, (ow - 1) * stride[1] - pad[1] + win[1] > W, pad != (0, 0)))
    assert (True, False, False) in over and (True, False, True) in over and (False, True, True) in over, over


@pytest.mark.parametrize("name", sorted(POOLS))
@pytest.mark.parametrize("floor_mode", [False, True])
def test_pooling_oracle_equals_numpy(name, floor_mode):
    """O.pool_i8_nhwc (s8, u8, the f32 output of the averages) and O.pool_f32_nchw == tests/asym_util.pool_reference, whose windows,
    divisors and output shape are written out per axis from the reference's sources; and the shape equals O.pool_out_hw"""
    case = POOLS[name]
    N, H, W, C, win, stride, pad = case
    shape = AU.pool_out_hw(case, floor_mode)
    assert shape == O.pool_out_hw(H, W, pad, win, stride, floor_mode)
    rng = np.random.default_rng(AU.seed_of(name, int(floor_mode)))
    for dt in (S8, U8):
        x = AU.rand8(rng, (N, H, W, C), dt)
        lo, hi = (-128, 127) if dt == S8 else (0, 255)
        for ptype in AU.POOL_TYPES:
            want = AU.pool_reference(x, case, ptype, floor_mode, False)
            got = O.pool_i8_nhwc(x, win, stride, pad, ptype, floor_mode=floor_mode)
            assert got.shape == want.shape == (N,) + shape + (C,)
            assert np.array_equal(got, np.clip(np.rint(want), lo, hi).astype(got.dtype)), (name, dt, ptype)
            if ptype:
                gf = O.pool_i8_nhwc(x, win, stride, pad, ptype, out_dtype=F32, floor_mode=floor_mode)
                assert np.array_equal(gf, want.astype(np.float32)), (name, dt, ptype, "f32 out")
    xf = (rng.random((N, C, H, W)) * 4.0 - 2.0).astype(np.float32)
    for ptype in AU.POOL_TYPES:
        want = AU.pool_reference(xf, case, ptype, floor_mode, True)
        got = O.pool_f32_nchw(xf, win, stride, pad, ptype, floor_mode=floor_mode)
        assert got.shape == want.shape
        if ptype == 0:
            assert np.array_equal(got, want.astype(np.float32)), (name, ptype)
        else:      # a float32 running sum against a float64 one: a few ulps of the largest partial sum
            assert np.abs(got - want).max() <= 1e-5 * max(np.abs(want).max(), 1.0), (name, ptype)


def test_pooling_divisors_clip_per_axis():
    """the including-padding average of the FP32 path on an image of ones IS window area / (bh * bw): where a window reaches past
    H + pad_h but not past W + pad_w the quotient shows that bh alone was clipped (and the mirror)"""
    for name, axis in (("w32_s21_p10_c10", 0), ("w23_s12_p01_c64", 1)):
        case = POOLS[name]
        N, H, W, C, win, stride, pad = case
        got = O.pool_f32_nchw(np.ones((N, C, H, W), np.float32), win, stride, pad, 1)
        oh, ow = AU.pool_out_hw(case, False)
        # last window of `axis`, an interior window of the other axis
        i, j = (oh - 1, 1) if axis == 0 else (1, ow - 1)
        start = (i * stride[0] - pad[0], j * stride[1] - pad[1])[axis]
        size = (H, W)[axis]
        inside = size - start
        clipped = min(start + win[axis], size + pad[axis]) - start
        assert inside < clipped < win[axis], (name, inside, clipped)
        other = win[1 - axis]
        assert got[0, 0, i, j] == np.float32(inside * other) / np.float32(clipped * other), (name, got[0, 0, i, j])


@needs_ref
@pytest.mark.parametrize("name", sorted(POOLS))
def test_int8_pooling_against_the_reference_helper(name):
    """pool_basic_check_int8 (conv_func_helper.h:29-100) where it is defined: s8 data >= 0 (it reads `char` and stores through an unsigned
    cast) and output shapes whose windows stay inside an UNPADDED axis (it clips only where pad > 0) - the floor shape, and the ceil
    shape where nothing hangs over. Max pooling is equal; the averages differ by at most one unit, rarely, because the helper divides where
    the kernel multiplies by a float32 reciprocal (tests/test_oracle_vs_ref.py pins that contract) - no divisor here is a power of two."""
    case = POOLS[name]
    N, H, W, C, win, stride, pad = case
    x = np.random.default_rng(AU.seed_of(name)).integers(0, 128, (N, H, W, C)).astype(np.int8)
    ran = 0
    for floor_mode in (True, False):
        oh, ow = AU.pool_out_hw(case, floor_mode)
        if any(pad[a] == 0 and ((oh, ow)[a] - 1) * stride[a] + win[a] > (H, W)[a] for a in range(2)):
            continue
        for ptype in AU.POOL_TYPES:
            got = O.pool_i8_nhwc(x, win, stride, pad, ptype, floor_mode=floor_mode).astype(np.int32)
            want = O.ref_pool_basic_check_int8(x, oh, ow, win, stride, pad, ptype).astype(np.int32)
            if ptype == 0:
                assert np.array_equal(got, want), (name, floor_mode)
            else:
                assert np.abs(got - want).max() <= 1 and (got != want).mean() < 0.02, (name, floor_mode, ptype, (got != want).mean())
        ran += 1
    assert ran >= 1


# ---- host-side selection ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def built():
    if not os.path.exists(L.LIB_PATH) or os.path.exists("/opt/rocm/bin/hipcc"):
        B.build()
    return L.load()


def _variants(forms):
    return {(code >> 16) & 0xff for code, _ in forms}


def _names(forms):
    return [n for _, n in forms]


# descriptors beside the table: C = 64 3x3 convs that differ from a halo-eligible one in ONE pair, and near-stems
_BESIDE = {
    "c64_s21":  (1, 10, 11, 64, 64, (3, 3), (1, 1), (2, 1), (1, 1), 1),
    "c64_s12":  (1, 10, 11, 64, 64, (3, 3), (1, 1), (1, 2), (1, 1), 1),
    "c64_d21":  (1, 10, 11, 64, 64, (3, 3), (2, 1), (1, 1), (2, 1), 1),
    "c64_d12":  (1, 10, 11, 64, 64, (3, 3), (1, 2), (1, 1), (1, 2), 1),
    "c64_3x1":  (1, 10, 11, 64, 64, (3, 1), (1, 0), (1, 1), (1, 1), 1),
    "c64_1x3":  (1, 10, 11, 64, 64, (1, 3), (0, 1), (1, 1), (1, 1), 1),
    "c64_p21":  (1, 10, 11, 64, 64, (3, 3), (2, 1), (1, 1), (1, 1), 1),
    "c3_7x7_s21": (1, 30, 27, 3, 64, (7, 7), (3, 2), (2, 1), (1, 1), 1),
    "c3_7x7_s12": (1, 30, 27, 3, 64, (7, 7), (3, 2), (1, 2), (1, 1), 1),
    "c3_7x5":   (1, 30, 27, 3, 64, (7, 5), (3, 2), (2, 2), (1, 1), 1),
    "c3_5x7":   (1, 30, 27, 3, 64, (5, 7), (2, 3), (2, 2), (1, 1), 1),
    "c3_7x7_d21": (1, 30, 27, 3, 64, (7, 7), (3, 2), (2, 2), (2, 1), 1),
}
HALO_CASES = {"p01", "p10", "img_p01", "img_p10"}
STEM_CASES = {"stem_p32", "stem_p23"}


def test_selection_of_per_axis_descriptors(built):
    """Which families accept which per-axis descriptor, from create() and set_tile() alone; a refused code changes nothing (asserted inside
    accepted_forms for every refused code). The accepted names are printed: tests/test_gpu_asym.py runs exactly these."""
    lib = built
    i8_codes, f32_codes = AU.selection_codes(True), AU.selection_codes(False)
    everything = dict(CASES, **_BESIDE)
    reached = set()
    for name in sorted(everything):
        case = everything[name]
        N, H, W, C, K, k, pad, stride, dil, g = case
        h = AU.create_conv(lib, L, case, True)
        forms = AU.accepted_forms(lib, h, i8_codes)
        names, variants = _names(forms), _variants(forms)
        print("%s %s INT8: %d forms: %s" % (name, case, len(forms), " ".join(names)))
        reached |= set(names)
        static = forms[0][1]
        # variants 16 / 17 (depthwise / grouped 3x3 kernels): refused on every per-axis descriptor; a grouped op stays on the direct kernel
        assert not (variants & {16, 17}), (name, names)
        assert not any(n.startswith(("dw3x3", "g3x3", "imgres")) for n in names), (name, names)
        for code in AU.DW_GROUP_CODES:
            assert lib.saber_hip_conv2d_set_tile(h, code) == -2, (name, hex(code))
        if g > 1:
            assert static == "direct_i8" and set(names) == {"direct_i8"}, (name, names)
        # halo (5, 6) and small-image (9) 3x3 kernels: pad (0, 1) / (1, 0) yes; unequal stride or dilation, another kernel size, pad 2: no
        halo = [n for n in names if n.startswith("halo3x3_i8")]
        img = [n for n in names if n.startswith("img3x3_i8")]
        if name in HALO_CASES:
            assert {"halo3x3_i8_4x16", "halo3x3_i8_8x16"} <= {n[:15] for n in halo}, (name, names)
        else:
            assert not halo and not img and not (variants & {5, 6, 9}), (name, names)
        if name.startswith("img_"):
            assert img, (name, names)
        # stem kernel (7): 7x7 with stride (2, 2) and dilation (1, 1) only - at any padding
        stem = [n for n in names if n.startswith("stem7x7s2_i8")]
        assert bool(stem) == (name in STEM_CASES), (name, names)
        if name in STEM_CASES:
            assert static.startswith("stem7x7s2_i8"), static
        # the NHWC4 path (C <= 4) has the register-staged implicit GEMM and nothing else beside the stem
        if C <= 4:
            assert all(n.startswith(("igemm_i8_c4", "stem7x7s2_i8")) for n in names) and any(n.startswith("igemm_i8_c4") for n in names), names
        elif g == 1:
            assert any("_dma" in n for n in names) and any(n.startswith("igemm_i8_") and "_dma" not in n for n in names), (name, names)
        lib.saber_hip_conv2d_destroy(h)

        # FP32, NHWC: the f32-MFMA implicit GEMM (or the direct kernel); variants 13 / 14 (bf16-plane halo and pointwise kernels), 16, 17 refused
        # (13 / 14 say nothing here: their planes are packed by set_weights, so without weights they refuse ANY descriptor; the check that
        # counts is the device one, test_fp32_table_every_accepted_form_within_tolerance, after set_weights)
        h = AU.create_conv(lib, L, case, False)
        forms = AU.accepted_forms(lib, h, f32_codes)
        names, variants = _names(forms), _variants(forms)
        print("%s FP32: %d forms: %s" % (name, len(forms), " ".join(names)))
        reached |= set(names)
        assert not (variants & {13, 14, 16, 17}), (name, names)
        assert not any(n.startswith(("halo3x3_f32", "pw1x1_f32", "dw3x3")) for n in names), (name, names)
        if g > 1 or C % 4:
            assert set(names) == {"direct_f32"}, (name, names)
        else:
            assert all(n.startswith("igemm_f32") for n in names) and any("_dma" in n for n in names), (name, names)
        lib.saber_hip_conv2d_destroy(h)
    for prefix in ("igemm_i8_", "igemm_i8_c4_", "halo3x3_i8_4x16", "halo3x3_i8_8x16", "img3x3_i8", "stem7x7s2_i8", "direct_i8", "igemm_f32_", "direct_f32"):
        assert any(n.startswith(prefix) for n in reached), (prefix, sorted(reached))


def test_fused_stem_pooling_accepts_any_conv_padding(built):
    """set_pooling asks for the stem kernel and the 3x3 / 2 unpadded max pooling, not for the conv's padding: pad (3, 2) and (2, 3) fuse,
    and the pooled shape is the per-axis one; a per-axis pooling window or stride does not fuse"""
    lib = built
    import ctypes as C
    for name in sorted(STEM_CASES):
        case = CASES[name]
        h = AU.create_conv(lib, L, case, True, in_dt=L.U8, out_dt=L.U8)
        for bad in ((3, 2, 2, 2), (3, 3, 2, 1), (2, 3, 2, 2), (3, 3, 1, 2)):
            assert lib.saber_hip_conv2d_set_pooling(h, L.POOL_MAX, bad[0], bad[1], bad[2], bad[3], 0, 0, 0) == L.UNIMPL, (name, bad)
        assert lib.saber_hip_conv2d_set_pooling(h, L.POOL_MAX, 3, 3, 2, 2, 1, 0, 0) == L.UNIMPL
        assert lib.saber_hip_conv2d_set_pooling(h, L.POOL_MAX, 3, 3, 2, 2, 0, 0, 0) == 0, lib.saber_hip_last_error()
        assert "maxpool" in lib.saber_hip_conv2d_algo(h).decode()
        oh, ow = C.c_int(), C.c_int()
        lib.saber_hip_conv2d_out_shape(h, C.byref(oh), C.byref(ow))
        ch, cw = AU.out_hw(case)
        assert (oh.value, ow.value) == O.pool_out_hw(ch, cw, (0, 0), (3, 3), (2, 2))
        lib.saber_hip_conv2d_destroy(h)
