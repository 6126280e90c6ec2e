"""Parity of the HIP path (through the C ABI) against the committed golden vectors and the CPU oracle.
INT8 / byte / index results must be BIT-EXACT; FP32 within 1e-4 relative (BASELINE.json north_star)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from anakin_amd import lib as L  # noqa: E402
from anakin_amd import saber as S  # noqa: E402
from oracle import oracle as O  # noqa: E402
from tests.golden_util import conv_f32_fixtures, conv_i8_fixtures, load  # noqa: E402

FP32_RTOL = 1e-4  # relative to max|reference| (tensor_cmp_host style, saber/core/tensor_op.cpp:580-600)


@pytest.fixture(scope="module", autouse=True)
def _device():
    L.require_device()  # fail loudly: no fallback path exists


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def run_conv_i8(x, w, w_scale, bias, in_scale, out_scale, out_dtype, relu, pad, stride, dil, group, tile=None,
                res_param=None, res=None, y_init=None):
    N, H, W, Cc = x.shape
    p = S.ConvParam(w, bias, group, (pad, pad), (stride, stride), (dil, dil), bool(relu), w_scale)
    if res_param:
        p.res_mode, p.res_relu, p.sum_scale, p.coeff, p.scale_res = res_param
    conv = S.SaberConv2D(int8=True).init((N, Cc, H, W), p, O.code_of(x), out_dtype, in_scale, out_scale)
    if tile is not None and conv.algo().startswith(("igemm", "stem", "halo")):
        conv.set_tile(tile)
    y = conv.new_output()
    if y_init is not None:
        y.copy_(dev(y_init))
    conv.dispatch(dev(x), y, None if res is None else dev(res))
    return host(y), conv


@pytest.mark.parametrize("name", conv_i8_fixtures())
def test_conv_i8_golden(name):
    g = load(name)
    N, H, W, C, K, k, pad, stride, dil, group, idt, odt, relu = [int(v) for v in g["spec"]]
    y, conv = run_conv_i8(g["x"], g["wq"], g["w_scale"], g["bias"], float(g["in_scale"]), float(g["out_scale"]),
                          odt, relu, pad, stride, dil, group)
    assert np.array_equal(y, g["y"]), conv.algo()
    if "w" in g.files:  # f32 weights in: the library quantises them (reference quirk: truncation)
        y2, conv2 = run_conv_i8(g["x"], g["w"], None, g["bias"], float(g["in_scale"]), float(g["out_scale"]),
                                odt, relu, pad, stride, dil, group)
        wq, ws = conv2.quantized_weights()
        assert np.array_equal(wq, g["wq"]) and np.array_equal(ws, g["w_scale"])
        assert np.array_equal(y2, g["y"])


@pytest.mark.parametrize("var", [1, 2])   # 1 = register-staged, 2 = LDS-DMA ring
@pytest.mark.parametrize("ks", [1, 2, 4])
@pytest.mark.parametrize("tile", range(len(L.TILES)))
@pytest.mark.parametrize("name", ["conv_i8_res2a_2b_3x3_u8u8", "conv_i8_res3a_2a_1x1s2_s8u8",
                                  "conv_i8_res4_2c_1x1_u8f32", "conv_i8_conv1_7x7s2_s8u8",
                                  "conv_i8_branch1_1x1s2_s8s8", "conv_i8_res5_2a_1x1_s8u8",
                                  "conv_i8_res5_2b_3x3_u8u8", "conv_i8_res2_2c_1x1_u8s8",
                                  "conv_i8_res5_2c_1x1_u8s8"])
def test_conv_i8_golden_every_tile(name, tile, ks, var):
    """Every (block tile, stage depth, staging) variant of the implicit-GEMM kernel reproduces the golden bytes."""
    g = load(name)
    N, H, W, C, K, k, pad, stride, dil, group, idt, odt, relu = [int(v) for v in g["spec"]]
    if C < 16 and var == 2:
        pytest.skip("first-layer (NHWC4) path is register-staged only")
    y, conv = run_conv_i8(g["x"], g["wq"], g["w_scale"], g["bias"], float(g["in_scale"]), float(g["out_scale"]),
                          odt, relu, pad, stride, dil, group, tile=tile | (ks << 8) | (var << 16))
    assert np.array_equal(y, g["y"]), conv.algo()
    assert conv.algo().endswith("_dma") == (var == 2)
    if var == 2 and ks == 4 and tile <= 2:   # intra-block split-K variants (2 / 4 wave groups)
        for v in ((3, 4) if tile == 0 else (3,)):
            y, conv = run_conv_i8(g["x"], g["wq"], g["w_scale"], g["bias"], float(g["in_scale"]),
                                  float(g["out_scale"]), odt, relu, pad, stride, dil, group,
                                  tile=tile | (ks << 8) | (v << 16))
            assert np.array_equal(y, g["y"]), conv.algo()


@pytest.mark.parametrize("var", [5, 6])   # LDS-halo 3x3 kernel, 4 / 8 tile rows
@pytest.mark.parametrize("combo", [(O.U8, O.U8, 1), (O.S8, O.S8, 0), (O.U8, O.F32, 0), (O.U8, O.S8, 1)])
@pytest.mark.parametrize("case", [(2, 56, 56, 64, 64, 1), (1, 28, 28, 128, 128, 1), (3, 14, 14, 256, 64, 1),
                                  (2, 7, 7, 512, 128, 1), (1, 19, 21, 64, 72, 1), (1, 10, 9, 128, 64, 0)])
def test_conv3x3_halo_vs_oracle(case, combo, var):
    N, H, W, C, K, pad = case
    idt, odt, relu = combo
    rng = np.random.default_rng(abs(hash((case, combo))) % 2**31)
    x = (rng.integers(0, 256, (N, H, W, C)).astype(np.uint8) if idt == O.U8
         else rng.integers(-128, 128, (N, H, W, C)).astype(np.int8))
    w = (rng.standard_normal((K, C, 3, 3)) * np.sqrt(2.0 / (C * 9))).astype(np.float32)
    b = (rng.standard_normal(K) * 0.5).astype(np.float32)
    in_scale, out_scale = 0.017, 0.041
    ws = O.weight_scales(w)
    wq = O.quant_weights(w, ws)
    bp, sc = O.conv_i8_prepare(ws, b, in_scale, out_scale, idt, odt)
    want = O.conv_i8(x, wq, bp, sc, odt, relu, (pad, pad))
    got, conv = run_conv_i8(x, w, None, b, in_scale, out_scale, odt, relu, pad, 1, 1, 1, tile=var << 16)
    assert conv.algo().startswith("halo3x3"), conv.algo()
    assert got.dtype == want.dtype and np.array_equal(got, want), conv.algo()


# small-image 3x3 kernel (conv3x3_img.h): (images per slab, rows per slab) variants over the ResNet 3x3 geometries
# + ragged / unpadded / partial-slab cases; every epilogue kind
IMG_CASES = [
    # N, H, W, C, K, pad, [(ib, rb), ...]
    (8, 14, 14, 256, 256, 1, [(1, 7), (1, 4), (1, 2)]),          # res4 branch2b
    (8, 7, 7, 512, 512, 1, [(1, 7), (2, 7), (2, 4), (4, 3)]),    # res5 branch2b
    (2, 28, 28, 128, 128, 1, [(1, 7), (1, 4), (2, 3), (1, 3)]),  # res3 branch2b
    (2, 56, 56, 64, 64, 1, [(1, 4), (1, 2), (2, 1)]),            # res2 branch2b
    (3, 7, 7, 512, 80, 1, [(2, 7), (3, 2)]),                     # ragged batch (3 images in slabs of 2 / 4), K % 16 = 0
    (5, 9, 11, 256, 40, 1, [(1, 4), (2, 2), (1, 9)]),            # odd sizes, rows not a multiple of the slab, K = 40
    (2, 10, 9, 128, 64, 0, [(1, 4), (2, 3)]),                    # no padding
    (1, 13, 13, 64, 24, 1, [(1, 7), (1, 13)]),                   # K not a multiple of 16
]


@pytest.mark.parametrize("combo", [(O.U8, O.U8, 1), (O.S8, O.S8, 0), (O.U8, O.F32, 0), (O.U8, O.S8, 1)])
@pytest.mark.parametrize("case", IMG_CASES)
def test_conv3x3_img_vs_oracle(case, combo):
    N, H, W, C, K, pad, slabs = case
    idt, odt, relu = combo
    rng = np.random.default_rng(abs(hash((case[:6], combo))) % 2**31)
    x = (rng.integers(0, 256, (N, H, W, C)).astype(np.uint8) if idt == O.U8
         else rng.integers(-128, 128, (N, H, W, C)).astype(np.int8))
    w = (rng.standard_normal((K, C, 3, 3)) * np.sqrt(2.0 / (C * 9))).astype(np.float32)
    b = (rng.standard_normal(K) * 0.5).astype(np.float32)
    in_scale, out_scale = 0.017, 0.041
    ws = O.weight_scales(w)
    wq = O.quant_weights(w, ws)
    bp, sc = O.conv_i8_prepare(ws, b, in_scale, out_scale, idt, odt)
    want = O.conv_i8(x, wq, bp, sc, odt, relu, (pad, pad))
    ran = 0
    for ib, rb in slabs:
        try:   # a slab beyond the kernel's LDS / row budget is refused by set_tile (the autotuner never offers it)
            got, conv = run_conv_i8(x, w, None, b, in_scale, out_scale, odt, relu, pad, 1, 1, 1,
                                    tile=rb | (ib << 8) | (9 << 16))
        except L.SaberHipError:
            continue
        ran += 1
        assert conv.algo().startswith("img3x3") and conv.algo().endswith("_w4"), conv.algo()
        assert got.dtype == want.dtype and np.array_equal(got, want), (conv.algo(), ib, rb)
    assert ran >= 1, case


def test_conv3x3_img_fused_eltwise_and_rejects():
    rng = np.random.default_rng(15)
    x = rng.integers(0, 256, (2, 14, 14, 256)).astype(np.uint8)
    w = (rng.standard_normal((64, 256, 3, 3)) * 0.04).astype(np.float32)
    b = (rng.standard_normal(64) * 0.5).astype(np.float32)
    res = rng.integers(-128, 128, (2, 14, 14, 64)).astype(np.int8)
    ws = O.weight_scales(w)
    bp, sc = O.conv_i8_prepare(ws, b, 0.02, 0.05, O.U8, O.S8)
    y1 = O.conv_i8(x, O.quant_weights(w, ws), bp, sc, O.S8, 0, (1, 1))
    want = O.eltwise_i8(y1, res, 0.05, 0.043, 20.0, 20.0, True)
    got, conv = run_conv_i8(x, w, None, b, 0.02, 0.05, O.S8, 0, 1, 1, 1, 1, tile=7 | (1 << 8) | (9 << 16),
                            res_param=(L.RES_ELTWISE, True, 1.0, (20.0, 20.0), 0.043), res=res)
    assert conv.algo().startswith("img3x3") and np.array_equal(got, want)
    # slabs beyond the LDS / accumulator budget, and non-3x3 geometry, are refused (the autotuner never offers them)
    p = S.ConvParam(w, b, 1, (1, 1), (1, 1), (1, 1), True)
    conv = S.SaberConv2D(True).init((2, 256, 14, 14), p, L.U8, L.U8, 0.02, 0.05)
    for bad in (14 | (1 << 8) | (9 << 16), 7 | (4 << 8) | (9 << 16)):
        with pytest.raises(L.SaberHipError):
            conv.set_tile(bad)
    p1 = S.ConvParam(w[:, :, :1, :1].copy(), b, 1, (0, 0), (1, 1), (1, 1), True)
    conv1 = S.SaberConv2D(True).init((2, 256, 14, 14), p1, L.U8, L.U8, 0.02, 0.05)
    with pytest.raises(L.SaberHipError):
        conv1.set_tile(7 | (1 << 8) | (9 << 16))


def test_conv3x3_halo_fused_eltwise():
    rng = np.random.default_rng(14)
    x = rng.integers(0, 256, (2, 28, 28, 128)).astype(np.uint8)
    w = (rng.standard_normal((128, 128, 3, 3)) * 0.05).astype(np.float32)
    b = (rng.standard_normal(128) * 0.5).astype(np.float32)
    res = rng.integers(-128, 128, (2, 28, 28, 128)).astype(np.int8)
    ws = O.weight_scales(w)
    bp, sc = O.conv_i8_prepare(ws, b, 0.02, 0.05, O.U8, O.S8)
    y1 = O.conv_i8(x, O.quant_weights(w, ws), bp, sc, O.S8, 0, (1, 1))
    want = O.eltwise_i8(y1, res, 0.05, 0.043, 20.0, 20.0, True)
    got, conv = run_conv_i8(x, w, None, b, 0.02, 0.05, O.S8, 0, 1, 1, 1, 1, tile=6 << 16,
                            res_param=(L.RES_ELTWISE, True, 1.0, (20.0, 20.0), 0.043), res=res)
    assert conv.algo().startswith("halo3x3") and np.array_equal(got, want)


@pytest.mark.parametrize("var", [1, 2])
@pytest.mark.parametrize("ks", [1, 2, 4])
@pytest.mark.parametrize("tile", range(len(L.TILES)))
def test_conv_f32_every_tile(tile, ks, var):
    g = load("conv_f32_3x3")
    N, C, H, W, K, k, pad, stride = [int(v) for v in g["spec"]]
    p = S.ConvParam(g["w"], g["bias"], 1, (pad, pad), (stride, stride), (1, 1), True)
    conv = S.SaberConv2D(int8=False).init((N, C, H, W), p, L.F32, L.F32)
    conv.set_tile(tile | (ks << 8) | (var << 16))
    y = conv.new_output()
    conv.dispatch(dev(g["x"]), y)
    err = np.abs(host(y) - g["y"]).max() / np.abs(g["y"]).max()
    assert err <= FP32_RTOL, (conv.algo(), err)


SWEEP = [
    # N, H, W, C, K, k, pad, stride, dil
    (3, 9, 9, 16, 20, 1, 0, 1, 1),     # K not a multiple of the tile / of 4-wide stores? (20 % 4 == 0)
    (1, 7, 7, 48, 34, 3, 1, 1, 1),     # K % 4 != 0 -> byte stores; C = 48 (K-step straddles taps)
    (2, 13, 11, 32, 64, 3, 1, 2, 1),   # ragged spatial, stride 2
    (1, 10, 10, 16, 16, 3, 2, 1, 2),   # dilation 2
    (1, 5, 5, 64, 32, 5, 2, 1, 1),     # 5x5
    (2, 1, 1, 128, 10, 1, 0, 1, 1),    # 1x1 spatial (fc-like), tiny M
    (1, 33, 17, 4, 24, 3, 1, 1, 1),    # C == 4 -> first-layer (C4) path
    (1, 16, 16, 3, 8, 7, 3, 2, 1),     # C == 3 -> padded to 4
    (1, 6, 6, 1, 8, 3, 1, 1, 1),       # C == 1
]


@pytest.mark.parametrize("case", SWEEP)
@pytest.mark.parametrize("combo", [(O.S8, O.S8, 0), (O.S8, O.U8, 1), (O.U8, O.S8, 0), (O.U8, O.U8, 1),
                                   (O.U8, O.F32, 0), (O.S8, O.F32, 1)])
def test_conv_i8_sweep_vs_oracle(case, combo):
    N, H, W, C, K, k, pad, stride, dil = case
    idt, odt, relu = combo
    rng = np.random.default_rng(abs(hash((case, combo))) % 2**31)
    x = (rng.integers(0, 256, (N, H, W, C)).astype(np.uint8) if idt == O.U8
         else rng.integers(-128, 128, (N, H, W, C)).astype(np.int8))
    w = (rng.standard_normal((K, C, k, k)) * np.sqrt(2.0 / (C * k * k))).astype(np.float32)
    b = (rng.standard_normal(K) * 0.5).astype(np.float32)
    in_scale, out_scale = 0.017, 0.041
    ws = O.weight_scales(w)
    wq = O.quant_weights(w, ws)
    bp, sc = O.conv_i8_prepare(ws, b, in_scale, out_scale, idt, odt)
    want = O.conv_i8(x, wq, bp, sc, odt, relu, (pad, pad), (stride, stride), (dil, dil))
    got, conv = run_conv_i8(x, w, None, b, in_scale, out_scale, odt, relu, pad, stride, dil, 1)
    assert got.dtype == want.dtype and np.array_equal(got, want), conv.algo()
    if conv.algo().startswith("igemm_i8_") and "_c4_" not in conv.algo():
        for tile, var in ((0, 2), (2, 2), (0, 3), (1, 3), (2, 3), (0, 4)):   # dma, dma + 2 / 4 wave groups
            got, conv = run_conv_i8(x, w, None, b, in_scale, out_scale, odt, relu, pad, stride, dil, 1,
                                    tile=tile | (4 << 8) | (var << 16))
            assert np.array_equal(got, want), conv.algo()


@pytest.mark.parametrize("combo", [(O.U8, O.U8, 1), (O.U8, O.S8, 0), (O.S8, O.S8, 1), (O.S8, O.U8, 0)])
def test_conv_i8_saturation_both_ends(combo):
    """Tiny out_scale: most outputs saturate at -128/127 or 0/255 (vpmovsdb/vpmovusdb semantics);
    exact .5 ties in the requantised value exercise round-to-nearest-even."""
    idt, odt, relu = combo
    rng = np.random.default_rng(77)
    x = (rng.integers(0, 256, (2, 9, 9, 32)).astype(np.uint8) if idt == O.U8
         else rng.integers(-128, 128, (2, 9, 9, 32)).astype(np.int8))
    wq = rng.integers(-127, 128, (64, 32, 3, 3)).astype(np.int8)
    ws = np.full(64, 0.5, np.float32)          # scale = 0.5*1/1 -> d = acc/2: half of the values are exact ties
    for out_scale in (1.0, 400.0):
        bp, sc = O.conv_i8_prepare(ws, None, 1.0, out_scale, idt, odt)
        want = O.conv_i8(x, wq, None, sc, odt, relu, (1, 1))
        got, conv = run_conv_i8(x, wq, ws, None, 1.0, out_scale, odt, relu, 1, 1, 1, 1)
        assert np.array_equal(got, want), (conv.algo(), out_scale)
        assert (want == (255 if odt == O.U8 else 127)).any() or out_scale > 1


def test_conv_i8_accumulators_beyond_2_pow_24():
    """|acc| far above 2^24: (float)acc must round like the CPU's int->float conversion (RNE), for every kernel
    family (implicit GEMM, LDS-DMA + wave groups, LDS-halo)."""
    rng = np.random.default_rng(5)
    x = rng.integers(200, 256, (1, 7, 7, 512)).astype(np.uint8)
    wq = rng.integers(100, 128, (64, 512, 3, 3)).astype(np.int8)
    ws = np.full(64, 1e-3, np.float32)
    acc = O.conv_i8_acc(x, wq, (1, 1))
    assert np.abs(acc).max() > 5 * 2**24
    for odt, out_scale in ((O.F32, 1.0), (O.S8, 900.0)):
        bp, sc = O.conv_i8_prepare(ws, None, 1.0, out_scale, O.U8, odt)
        want = O.conv_i8(x, wq, None, sc, odt, 0, (1, 1))
        for tile in (None, 2 | (4 << 8) | (1 << 16), 0 | (4 << 8) | (4 << 16), 6 << 16):
            got, conv = run_conv_i8(x, wq, ws, None, 1.0, out_scale, odt, 0, 1, 1, 1, 1, tile=tile)
            assert np.array_equal(got, want), conv.algo()


def test_conv_rejects_unknown_activation():
    d = L.ConvDesc()
    d.n, d.h, d.w, d.c, d.k, d.kh, d.kw = 1, 8, 8, 16, 16, 1, 1
    d.stride_h = d.stride_w = d.dil_h = d.dil_w = d.group = 1
    d.in_dtype, d.out_dtype, d.in_layout, d.out_layout, d.int8_weights = L.U8, L.U8, L.NHWC, L.NHWC, 1
    d.act = 5   # e.g. a sigmoid: not fused, must not be silently dropped
    import ctypes as C
    h = C.c_void_p()
    assert L.load().saber_hip_conv2d_create(C.byref(d), C.byref(h)) == L.UNIMPL


def test_conv_i8_empty_and_invalid():
    lib = L.load()
    import ctypes as C
    d = L.ConvDesc()
    d.n, d.h, d.w, d.c, d.k, d.kh, d.kw = 1, 2, 2, 16, 16, 3, 3   # 3x3 on 2x2 without padding: empty output
    d.stride_h = d.stride_w = d.dil_h = d.dil_w = d.group = 1
    d.in_dtype, d.out_dtype, d.int8_weights = L.S8, L.S8, 1
    h = C.c_void_p()
    assert lib.saber_hip_conv2d_create(C.byref(d), C.byref(h)) == -2
    # run before set_weights must fail loudly, not silently compute
    d.pad_h = d.pad_w = 1
    assert lib.saber_hip_conv2d_create(C.byref(d), C.byref(h)) == 0
    x = torch.zeros(64, dtype=torch.int8, device="cuda")
    assert lib.saber_hip_conv2d_run(h, C.c_void_p(x.data_ptr()), C.c_void_p(x.data_ptr()), None, None, None) == -2
    lib.saber_hip_conv2d_destroy(h)


@pytest.mark.parametrize("combo", [(O.S8, O.U8, 1), (O.U8, O.U8, 1), (O.S8, O.S8, 0), (O.U8, O.F32, 0)])
@pytest.mark.parametrize("case", [(2, 64, 64, 3, 64, 3), (1, 37, 45, 4, 64, 3), (1, 30, 30, 1, 24, 2), (2, 224, 224, 3, 64, 3)])
def test_conv_stem_vs_oracle(case, combo):
    """The LDS-patch stem kernel (7x7 stride 2, <= 4 channels) against the oracle, and against the
    implicit-GEMM first-layer path it replaces."""
    N, H, W, C, K, pad = case
    idt, odt, relu = combo
    rng = np.random.default_rng(abs(hash((case, combo))) % 2**31)
    x = (rng.integers(0, 256, (N, H, W, C)).astype(np.uint8) if idt == O.U8
         else rng.integers(-128, 128, (N, H, W, C)).astype(np.int8))
    w = (rng.standard_normal((K, C, 7, 7)) * 0.1).astype(np.float32)
    b = (rng.standard_normal(K) * 0.5).astype(np.float32)
    ws = O.weight_scales(w)
    bp, sc = O.conv_i8_prepare(ws, b, 0.017, 0.08, idt, odt)
    want = O.conv_i8(x, O.quant_weights(w, ws), bp, sc, odt, relu, (pad, pad), (2, 2))
    got, conv = run_conv_i8(x, w, None, b, 0.017, 0.08, odt, relu, pad, 2, 1, 1, tile=7 << 16)
    assert conv.algo().startswith("stem7x7s2"), conv.algo()
    assert np.array_equal(got, want)
    got, conv = run_conv_i8(x, w, None, b, 0.017, 0.08, odt, relu, pad, 2, 1, 1, tile=8 << 16)
    assert conv.algo().startswith("igemm_i8_c4"), conv.algo()
    assert np.array_equal(got, want)


@pytest.mark.parametrize("case", [(2, 224, 224, 64, "f32"), (1, 61, 47, 64, "f32"), (2, 33, 40, 72, "s8"),
                                  (1, 30, 30, 64, "u8"), (1, 18, 23, 16, "f32")])
@pytest.mark.parametrize("odt", [O.U8, O.S8])
def test_conv_pooling_stem_fused_vs_oracle(case, odt):
    """SaberConv2DPooling: 7x7/2 stem + 3x3/2 max pooling in one kernel == oracle conv followed by oracle pooling,
    byte for byte (f32 image quantised on entry / s8 / u8 NHWC inputs, ragged sizes, ceil-mode windows clipped)."""
    N, H, W, K, kind = case
    rng = np.random.default_rng(abs(hash((case, odt))) % 2**31)
    w = (rng.standard_normal((K, 3, 7, 7)) * 0.1).astype(np.float32)
    b = (rng.standard_normal(K) * 0.3).astype(np.float32)
    in_scale, out_scale = 1 / 127.0, 0.02
    relu = odt == O.U8
    if kind == "f32":
        xf = rng.uniform(-1, 1, (N, 3, H, W)).astype(np.float32)
        xq = O.quant_nchw_to_nhwc(xf, in_scale, O.S8)
        x_dev, idt, in_layout = dev(xf), L.F32, L.NCHW
    else:
        xq = (rng.integers(0, 256, (N, H, W, 3)).astype(np.uint8) if kind == "u8"
              else rng.integers(-128, 128, (N, H, W, 3)).astype(np.int8))
        x_dev, idt, in_layout = dev(xq), O.code_of(xq), L.NHWC
    ws = O.weight_scales(w)
    bp, sc = O.conv_i8_prepare(ws, b, in_scale, out_scale, O.code_of(xq), odt)
    conv_out = O.conv_i8(xq, O.quant_weights(w, ws), bp, sc, odt, relu, (3, 3), (2, 2))
    want = O.pool_i8_nhwc(conv_out, (3, 3), (2, 2), (0, 0), 0)
    p = S.ConvParam(w, b, 1, (3, 3), (2, 2), (1, 1), relu)
    cp = S.SaberConv2DPooling().init((N, 3, H, W), p, L.POOL_MAX, (3, 3), (2, 2), (0, 0), idt, odt, in_scale,
                                     out_scale, in_layout=in_layout)
    assert cp.fused and "maxpool" in cp.algo()
    y = cp.new_output()
    y.fill_(9)
    cp.dispatch(x_dev, y)
    got = host(y)
    assert got.shape == want.shape and got.dtype == want.dtype and np.array_equal(got, want), cp.algo()


@pytest.mark.parametrize("case", [(2, 224, 224, "f32"), (1, 61, 47, "f32"), (2, 33, 40, "s8"), (1, 30, 30, "u8"), (3, 18, 23, "f32")])
@pytest.mark.parametrize("combo", [(O.U8, 256, 64), (O.S8, 64, 256), (O.U8, 32, 96)])
def test_stem_pool_pair_equals_the_three_ops(case, combo):
    """saber_hip_conv2d_stem_pair_create: conv1 + pool1 and the two 1x1 convs reading pool1 (res2a_branch1 / res2a_branch2a) in ONE
    launch == oracle conv -> pooling -> the two convs, byte for byte (ragged pooled sizes, every input form of the stem, s8 / u8 pooled
    tensors, both output types on either side); the pooled tensor itself is written only on request."""
    N, H, W, kind = case
    odt, K1, K2 = combo
    rng = np.random.default_rng(abs(hash((case, combo))) % 2**31)
    w = (rng.standard_normal((64, 3, 7, 7)) * 0.1).astype(np.float32)
    b = (rng.standard_normal(64) * 0.3).astype(np.float32)
    in_scale, pool_scale = 1 / 127.0, 0.02
    if kind == "f32":
        xf = rng.uniform(-1, 1, (N, 3, H, W)).astype(np.float32)
        xq = O.quant_nchw_to_nhwc(xf, in_scale, O.S8)
        x_dev, idt, in_layout = dev(xf), L.F32, L.NCHW
    else:
        xq = (rng.integers(0, 256, (N, H, W, 3)).astype(np.uint8) if kind == "u8" else rng.integers(-128, 128, (N, H, W, 3)).astype(np.int8))
        x_dev, idt, in_layout = dev(xq), O.code_of(xq), L.NHWC
    ws = O.weight_scales(w)
    bp, sc = O.conv_i8_prepare(ws, b, in_scale, pool_scale, O.code_of(xq), odt)
    pooled = O.pool_i8_nhwc(O.conv_i8(xq, O.quant_weights(w, ws), bp, sc, odt, odt == O.U8, (3, 3), (2, 2)), (3, 3), (2, 2), (0, 0), 0)
    stem = S.SaberConv2DPooling().init((N, 3, H, W), S.ConvParam(w, b, 1, (3, 3), (2, 2), (1, 1), odt == O.U8), L.POOL_MAX, (3, 3), (2, 2),
                                       (0, 0), idt, odt, in_scale, pool_scale, in_layout=in_layout)
    assert stem.fused
    ph, pw = pooled.shape[1:3]
    convs, wants = [], []
    for K, kdt, relu, out_scale in ((K1, O.S8, 0, 0.05), (K2, O.U8, 1, 0.031)):
        wk = (rng.standard_normal((K, 64, 1, 1)) * np.sqrt(2.0 / 64)).astype(np.float32)
        bk = (rng.standard_normal(K) * 0.5).astype(np.float32)
        wsk = O.weight_scales(wk)
        bpk, sck = O.conv_i8_prepare(wsk, bk, pool_scale, out_scale, odt, kdt)
        wants.append(O.conv_i8(pooled, O.quant_weights(wk, wsk), bpk, sck, kdt, relu))
        convs.append(S.SaberConv2D(True).init((N, 64, ph, pw), S.ConvParam(wk, bk, 1, (0, 0), (1, 1), (1, 1), bool(relu)), odt, kdt,
                                              pool_scale, out_scale))
    sp = S.SaberStemPair(stem, convs[0], convs[1])
    for with_pool in (True, False):
        ya, yb, yp = convs[0].new_output(), convs[1].new_output(), stem.new_output()
        ya.fill_(77)
        yb.fill_(77)
        yp.fill_(9)
        sp.dispatch(x_dev, ya, yb, yp if with_pool else None)
        assert np.array_equal(host(ya), wants[0]) and np.array_equal(host(yb), wants[1]), (case, combo, with_pool)
        assert np.array_equal(host(yp), pooled) if with_pool else bool((host(yp) == 9).all())
    # the three operators stay usable on their own
    yp = stem.new_output()
    stem.dispatch(x_dev, yp)
    ya = convs[0].new_output()
    convs[0].dispatch(yp, ya)
    assert np.array_equal(host(yp), pooled) and np.array_equal(host(ya), wants[0])


def test_stem_pool_pair_rejects_what_it_cannot_run():
    rng = np.random.default_rng(5)

    def stem(k):
        w = (rng.standard_normal((k, 3, 7, 7)) * 0.1).astype(np.float32)
        return S.SaberConv2DPooling().init((1, 3, 64, 64), S.ConvParam(w, None, 1, (3, 3), (2, 2), (1, 1), True), L.POOL_MAX, (3, 3), (2, 2),
                                           (0, 0), L.F32, O.U8, 1 / 127.0, 0.02, in_layout=L.NCHW)

    def conv(k, c=64, hw=16, idt=O.U8, kk=1):
        w = (rng.standard_normal((k, c, kk, kk)) * 0.1).astype(np.float32)
        return S.SaberConv2D(True).init((1, c, hw, hw), S.ConvParam(w, None, 1, (kk // 2, kk // 2), (1, 1), (1, 1), True), idt, O.U8, 0.02, 0.05)

    st = stem(64)
    S.SaberStemPair(st, conv(256), conv(64))
    for bad in (lambda: S.SaberStemPair(st, conv(256), conv(48)),              # k % 32
                lambda: S.SaberStemPair(st, conv(256), conv(96)),              # k_a + k_b > 320
                lambda: S.SaberStemPair(st, conv(256), conv(64, hw=15)),       # not the pooled tensor's shape
                lambda: S.SaberStemPair(st, conv(256), conv(64, idt=O.S8)),    # reads s8, the stem writes u8
                lambda: S.SaberStemPair(st, conv(256), conv(64, kk=3)),        # not 1x1
                lambda: S.SaberStemPair(conv(64), conv(256), conv(64))):       # the head is not a fused conv + pooling
        with pytest.raises(L.SaberHipError):
            bad()


def test_conv_pooling_unfused_fallback_is_two_ops():
    """No fused kernel for this combination: conv into an inner tensor, then pooling (SaberConv2DPooling<X86,AK_FLOAT>
    structure); same bytes as the oracle."""
    rng = np.random.default_rng(12)
    x = rng.integers(0, 256, (2, 14, 14, 32)).astype(np.uint8)
    w = (rng.standard_normal((64, 32, 3, 3)) * 0.1).astype(np.float32)
    ws = O.weight_scales(w)
    bp, sc = O.conv_i8_prepare(ws, None, 0.02, 0.05, O.U8, O.U8)
    want = O.pool_i8_nhwc(O.conv_i8(x, O.quant_weights(w, ws), None, sc, O.U8, 1, (1, 1)), (2, 2), (2, 2), (0, 0), 0)
    cp = S.SaberConv2DPooling().init((2, 32, 14, 14), S.ConvParam(w, None, 1, (1, 1), (1, 1), (1, 1), True),
                                     L.POOL_MAX, (2, 2), (2, 2), (0, 0), O.U8, O.U8, 0.02, 0.05)
    assert not cp.fused
    y = cp.new_output()
    assert np.array_equal(host(cp.dispatch(dev(x), y)), want)


def test_conv_i8_f32_input_quantises_on_entry():
    """SaberConv2D<X86,AK_INT8> handed an f32 NCHW tensor (first layer): reorder_nhwc_nchw then conv."""
    rng = np.random.default_rng(11)
    x = rng.uniform(-1, 1, (2, 3, 32, 32)).astype(np.float32)
    w = (rng.standard_normal((64, 3, 7, 7)) * 0.1).astype(np.float32)
    b = (rng.standard_normal(64) * 0.1).astype(np.float32)
    in_scale, out_scale = 1.0 / 127, 0.02
    p = S.ConvParam(w, b, 1, (3, 3), (2, 2), (1, 1), True)
    conv = S.SaberConv2D(True).init(x.shape, p, L.F32, L.U8, in_scale, out_scale, in_layout=L.NCHW)
    y = conv.new_output()
    conv.dispatch(dev(x), y)
    xq = O.quant_nchw_to_nhwc(x, in_scale, O.S8)
    ws = O.weight_scales(w)
    bp, sc = O.conv_i8_prepare(ws, b, in_scale, out_scale, O.S8, O.U8)
    want = O.conv_i8(xq, O.quant_weights(w, ws), bp, sc, O.U8, 1, (3, 3), (2, 2))
    assert conv.algo() == "stem7x7s2_i8_8x16_fusedquant"
    assert np.array_equal(host(y), want), conv.algo()
    conv.set_tile(8 << 16)   # the unfused path: quantise kernel + NHWC4 implicit GEMM
    y.zero_()
    conv.dispatch(dev(x), y)
    assert conv.algo().startswith("igemm_i8_c4") and np.array_equal(host(y), want)
    # values exactly on .5 ties and beyond the int8 range quantise like reorder_nhwc_nchw
    x2 = x.copy()
    x2[0, :, 0, :6] = np.array([0.5, 1.5, -0.5, -2.5, 300.0, -300.0], np.float32) * np.float32(in_scale)
    conv.set_tile(7 << 16)
    conv.dispatch(dev(x2), y)
    want2 = O.conv_i8(O.quant_nchw_to_nhwc(x2, in_scale, O.S8), O.quant_weights(w, ws), bp, sc, O.U8, 1, (3, 3), (2, 2))
    assert np.array_equal(host(y), want2)


@pytest.mark.parametrize("relu", [0, 1])
def test_conv_i8_fused_eltwise_equals_two_ops(relu):
    """RES_ELTWISE == conv(->s8) followed by SaberEltwise<AK_INT8> sum(+relu), bit for bit."""
    rng = np.random.default_rng(12)
    x = rng.integers(0, 256, (2, 14, 14, 64)).astype(np.uint8)
    w = (rng.standard_normal((256, 64, 1, 1)) * 0.15).astype(np.float32)
    b = (rng.standard_normal(256) * 0.5).astype(np.float32)
    res = rng.integers(-128, 128, (2, 14, 14, 256)).astype(np.int8)
    in_scale, out_scale, s_res, s_out = 0.02, 0.05, 0.043, 0.06
    c = 1.0 / s_out
    ws = O.weight_scales(w)
    wq = O.quant_weights(w, ws)
    bp, sc = O.conv_i8_prepare(ws, b, in_scale, out_scale, O.U8, O.S8)
    y1 = O.conv_i8(x, wq, bp, sc, O.S8, 0)
    want = O.eltwise_i8(y1, res, out_scale, s_res, c, c, relu)
    got, conv = run_conv_i8(x, w, None, b, in_scale, out_scale, O.S8, 0, 0, 1, 1, 1,
                            res_param=(L.RES_ELTWISE, bool(relu), 1.0, (c, c), s_res), res=res)
    assert np.array_equal(got, want), conv.algo()
    # every tile / staging variant
    for var, ks, tiles in ((1, 1, range(len(L.TILES))), (2, 1, range(len(L.TILES))), (3, 4, (0, 1, 2)), (4, 4, (0,))):
        for tile in tiles:
            got, conv = run_conv_i8(x, w, None, b, in_scale, out_scale, O.S8, 0, 0, 1, 1, 1,
                                    tile=tile | (ks << 8) | (var << 16),
                                    res_param=(L.RES_ELTWISE, bool(relu), 1.0, (c, c), s_res), res=res)
            assert np.array_equal(got, want), conv.algo()
    # and the unfused device ops agree too
    y1d, _ = run_conv_i8(x, w, None, b, in_scale, out_scale, O.S8, 0, 0, 1, 1, 1)
    assert np.array_equal(y1d, y1)
    e = S.eltwise_sum(dev(y1d), dev(res), (c, c), bool(relu), out_scale, s_res)
    assert np.array_equal(host(e), want)


CHAIN_CASES = [
    # C, N, HW, in dtype of the first conv, out dtype / relu of the second, eltwise relu, pixel fragments (None: default)
    (64, 2, 56, O.U8, O.U8, 1, 1, None),
    (64, 1, 13, O.U8, O.U8, 1, 1, 2),      # 169 pixels: ragged last tile
    (64, 1, 9, O.S8, O.S8, 0, 0, 4),       # s8 in, second conv without relu -> s8, eltwise without relu
    (128, 2, 28, O.U8, O.U8, 1, 1, None),
    (128, 1, 11, O.U8, O.S8, 1, 1, 1),
    (256, 2, 14, O.U8, O.U8, 1, 1, None),
    (256, 1, 5, O.S8, O.U8, 1, 0, None),   # 25 pixels
    (512, 2, 7, O.U8, O.U8, 1, 1, None),
    (512, 1, 3, O.U8, O.S8, 0, 1, None),
    (256, 2, 14, O.U8, O.U8, 1, 1, 9),     # second conv split over two workgroups
    (256, 1, 5, O.S8, O.S8, 0, 0, 9),
    (512, 2, 7, O.U8, O.U8, 1, 1, 9),
    (256, 2, 14, O.U8, O.U8, 1, 1, 11),    # split + 8 waves per workgroup
    (256, 1, 5, O.S8, O.S8, 0, 0, 11),
    (128, 2, 28, O.U8, O.U8, 1, 1, 6),     # 8 waves per workgroup
    (128, 1, 11, O.U8, O.S8, 1, 1, 5),
]


@pytest.mark.parametrize("case", CHAIN_CASES)
def test_conv1x1_chain_equals_two_launches_and_oracle(case):
    """saber_hip_conv2d_chain_run == [conv 1x1 + SaberEltwise sum] then [conv 1x1], bit for bit (both outputs)."""
    Cc, N, HW, idt, odt2, relu2, res_relu, tn = case
    rng = np.random.default_rng(1000 + Cc + HW)
    K1, K2 = 4 * Cc, Cc
    x = (rng.integers(0, 256, (N, HW, HW, Cc)).astype(np.uint8) if idt == O.U8
         else rng.integers(-128, 128, (N, HW, HW, Cc)).astype(np.int8))
    res = rng.integers(-128, 128, (N, HW, HW, K1)).astype(np.int8)
    w1 = (rng.standard_normal((K1, Cc, 1, 1)) * np.sqrt(2.0 / Cc)).astype(np.float32)
    b1 = (rng.standard_normal(K1) * 0.5).astype(np.float32)
    w2 = (rng.standard_normal((K2, K1, 1, 1)) * np.sqrt(2.0 / K1)).astype(np.float32)
    b2 = (rng.standard_normal(K2) * 0.5).astype(np.float32)
    s_in, s_mid, s_res, s_sum, s_out = 0.02, 0.05, 0.043, 0.06, 0.031
    c = 1.0 / s_sum
    # oracle
    ws1 = O.weight_scales(w1)
    bp1, sc1 = O.conv_i8_prepare(ws1, b1, s_in, s_mid, idt, O.S8)
    t = O.conv_i8(x, O.quant_weights(w1, ws1), bp1, sc1, O.S8, 0)
    want1 = O.eltwise_i8(t, res, s_mid, s_res, c, c, bool(res_relu))
    ws2 = O.weight_scales(w2)
    bp2, sc2 = O.conv_i8_prepare(ws2, b2, s_sum, s_out, O.S8, odt2)
    want2 = O.conv_i8(want1, O.quant_weights(w2, ws2), bp2, sc2, odt2, relu2)
    # device: two launches
    pa = S.ConvParam(w1, b1, 1, (0, 0), (1, 1), (1, 1), False)
    pa.res_mode, pa.res_relu, pa.sum_scale, pa.coeff, pa.scale_res = L.RES_ELTWISE, bool(res_relu), 1.0, (c, c), s_res
    ca = S.SaberConv2D(int8=True).init((N, Cc, HW, HW), pa, idt, O.S8, s_in, s_mid)
    pb = S.ConvParam(w2, b2, 1, (0, 0), (1, 1), (1, 1), bool(relu2))
    cb = S.SaberConv2D(int8=True).init((N, K1, HW, HW), pb, O.S8, odt2, s_sum, s_out)
    y1, y2 = ca.new_output(), cb.new_output()
    ca.dispatch(dev(x), y1, dev(res))
    cb.dispatch(y1, y2)
    assert np.array_equal(host(y1), want1) and np.array_equal(host(y2), want2)
    # device: one launch
    chain = S.SaberConvChain(ca, cb)
    if tn is not None:
        chain.set_tile(tn)
    z1, z2 = ca.new_output(), cb.new_output()
    z1.fill_(77)
    z2.fill_(77)
    chain.dispatch(dev(x), dev(res), z1, z2)
    assert np.array_equal(host(z1), want1), ("y1", chain.tile())
    assert np.array_equal(host(z2), want2), ("y2", chain.tile())


CHAIN3_CASES = [
    # C, N, H, W, dtype into the 3x3, dtype 3x3 -> first 1x1, out dtype / relu of the last conv, eltwise relu, tile rows
    (64, 2, 56, 56, O.U8, O.U8, O.U8, 1, 1, None),
    (64, 1, 13, 21, O.U8, O.U8, O.U8, 1, 1, 2),     # ragged rows and columns
    (64, 1, 7, 9, O.S8, O.S8, O.S8, 0, 0, 4),
    (128, 2, 28, 28, O.U8, O.U8, O.U8, 1, 1, None),
    (128, 1, 5, 17, O.U8, O.S8, O.U8, 1, 1, 1),
    (256, 2, 14, 14, O.U8, O.U8, O.U8, 1, 1, None),
    (256, 1, 3, 5, O.S8, O.U8, O.S8, 0, 1, None),
    (128, 2, 28, 28, O.U8, O.U8, O.U8, 1, 1, 5),    # 8 waves per workgroup
    (128, 1, 5, 17, O.U8, O.S8, O.U8, 1, 1, 6),
    (256, 2, 14, 14, O.U8, O.U8, O.U8, 1, 1, 3),    # C = 256, 8 waves per workgroup
    (256, 1, 3, 5, O.S8, O.U8, O.S8, 0, 1, 3),
    (256, 8, 14, 14, O.U8, O.U8, O.U8, 1, 1, 7),    # C = 256, two cooperating workgroups per tile (conv_chain_coop.hip): res4 at batch 8
    (256, 2, 14, 14, O.U8, O.U8, O.U8, 1, 1, 7),
    (256, 1, 3, 5, O.S8, O.U8, O.S8, 0, 1, 7),      # ragged: 3 tiles of 5 columns
    (256, 3, 5, 37, O.U8, O.S8, O.U8, 1, 0, 7),     # three column tiles per row, the last one ragged
    (256, 8, 14, 14, O.U8, O.U8, O.U8, 1, 1, 15),   # C = 256, FOUR cooperating workgroups per tile of 2 rows x 16 columns: res4 at batch 8
    (256, 2, 14, 14, O.U8, O.U8, O.U8, 1, 1, 15),
    (256, 1, 3, 5, O.S8, O.U8, O.S8, 0, 1, 15),     # ragged: an odd row count (the last tile's second row is outside the image)
    (256, 3, 5, 37, O.U8, O.S8, O.U8, 1, 0, 15),    # three column tiles per row pair, the last one ragged
    (256, 16, 14, 14, O.U8, O.U8, O.U8, 1, 1, 15),  # 448 workgroups: more than one per CU
]


@pytest.mark.parametrize("case", CHAIN3_CASES)
def test_conv3x3_chain_equals_three_launches_and_oracle(case):
    """saber_hip_conv2d_chain_create3: 3x3 conv -> [1x1 conv + SaberEltwise sum] -> 1x1 conv in one launch, bit for bit."""
    Cc, N, H, Wd, idt, mdt, odt2, relu2, res_relu, tn = case
    rng = np.random.default_rng(2000 + Cc + H)
    K1, K2 = 4 * Cc, Cc
    x = (rng.integers(0, 256, (N, H, Wd, Cc)).astype(np.uint8) if idt == O.U8
         else rng.integers(-128, 128, (N, H, Wd, Cc)).astype(np.int8))
    res = rng.integers(-128, 128, (N, H, Wd, K1)).astype(np.int8)
    w0 = (rng.standard_normal((Cc, Cc, 3, 3)) * np.sqrt(2.0 / (9 * Cc))).astype(np.float32)
    b0 = (rng.standard_normal(Cc) * 0.5).astype(np.float32)
    w1 = (rng.standard_normal((K1, Cc, 1, 1)) * np.sqrt(2.0 / Cc)).astype(np.float32)
    b1 = (rng.standard_normal(K1) * 0.5).astype(np.float32)
    w2 = (rng.standard_normal((K2, K1, 1, 1)) * np.sqrt(2.0 / K1)).astype(np.float32)
    b2 = (rng.standard_normal(K2) * 0.5).astype(np.float32)
    s_x, s_in, s_mid, s_res, s_sum, s_out = 0.023, 0.02, 0.05, 0.043, 0.06, 0.031
    c = 1.0 / s_sum
    relu0 = mdt == O.U8
    # oracle
    ws0 = O.weight_scales(w0)
    bp0, sc0 = O.conv_i8_prepare(ws0, b0, s_x, s_in, idt, mdt)
    t0 = O.conv_i8(x, O.quant_weights(w0, ws0), bp0, sc0, mdt, int(relu0), (1, 1))
    ws1 = O.weight_scales(w1)
    bp1, sc1 = O.conv_i8_prepare(ws1, b1, s_in, s_mid, mdt, O.S8)
    t1 = O.conv_i8(t0, O.quant_weights(w1, ws1), bp1, sc1, O.S8, 0)
    want1 = O.eltwise_i8(t1, res, s_mid, s_res, c, c, bool(res_relu))
    ws2 = O.weight_scales(w2)
    bp2, sc2 = O.conv_i8_prepare(ws2, b2, s_sum, s_out, O.S8, odt2)
    want2 = O.conv_i8(want1, O.quant_weights(w2, ws2), bp2, sc2, odt2, relu2)
    # device ops
    c0 = S.SaberConv2D(int8=True).init((N, Cc, H, Wd), S.ConvParam(w0, b0, 1, (1, 1), (1, 1), (1, 1), bool(relu0)), idt, mdt,
                                       s_x, s_in)
    pa = S.ConvParam(w1, b1, 1, (0, 0), (1, 1), (1, 1), False)
    pa.res_mode, pa.res_relu, pa.sum_scale, pa.coeff, pa.scale_res = L.RES_ELTWISE, bool(res_relu), 1.0, (c, c), s_res
    ca = S.SaberConv2D(int8=True).init((N, Cc, H, Wd), pa, mdt, O.S8, s_in, s_mid)
    cb = S.SaberConv2D(int8=True).init((N, K1, H, Wd), S.ConvParam(w2, b2, 1, (0, 0), (1, 1), (1, 1), bool(relu2)), O.S8, odt2,
                                       s_sum, s_out)
    y0, y1, y2 = c0.new_output(), ca.new_output(), cb.new_output()
    c0.dispatch(dev(x), y0)
    ca.dispatch(y0, y1, dev(res))
    cb.dispatch(y1, y2)
    assert np.array_equal(host(y0), t0) and np.array_equal(host(y1), want1) and np.array_equal(host(y2), want2)
    chain = S.SaberConvChain(ca, cb, conv3x3=c0)
    if tn is not None:
        chain.set_tile(tn)
    z1, z2 = ca.new_output(), cb.new_output()
    z1.fill_(77)
    z2.fill_(77)
    for rep in range(3 if tn in (7, 15) else 1):  # (the cooperative forms' arrival counters are never reset: launch after launch)
        z1.fill_(77)
        z2.fill_(77)
        chain.dispatch(dev(x), dev(res), z1, z2)
        assert chain.tile() == (tn if tn is not None else chain.tile())
        assert np.array_equal(host(z1), want1), ("y1", chain.tile(), rep)
        assert np.array_equal(host(z2), want2), ("y2", chain.tile(), rep)
    # conv3x3 + first 1x1 conv only (the last block of a stage: no 1x1 conv follows on the same pixels)
    double = S.SaberConvChain(ca, None, conv3x3=c0)
    if tn is not None and tn not in (7, 15):
        double.set_tile(tn)
    z1.fill_(55)
    double.dispatch(dev(x), dev(res), z1)
    assert np.array_equal(host(z1), want1), ("double y1", double.tile())


def _res4_blocks(rng, N, H, Wd, nblk, first_u8=True, Cc=256):
    """nblk ResNet res4 (C = 256) / res3 (C = 128) block chains: [3x3 -> 1x1 expand + eltwise(relu) -> next block's 1x1 reduce],
    chain i + 1 reading chain i's outputs; returns the device ops, the first inputs and the oracle's outputs per block."""
    K1 = 4 * Cc
    x = rng.integers(0, 256, (N, H, Wd, Cc)).astype(np.uint8) if first_u8 else rng.integers(-128, 128, (N, H, Wd, Cc)).astype(np.int8)
    res = rng.integers(-128, 128, (N, H, Wd, K1)).astype(np.int8)
    ops, wants = [], []
    cur_x, cur_res, idt = x, res, (O.U8 if first_u8 else O.S8)
    for k in range(nblk):
        w0 = (rng.standard_normal((Cc, Cc, 3, 3)) * np.sqrt(2.0 / (9 * Cc))).astype(np.float32)
        b0 = (rng.standard_normal(Cc) * 0.5).astype(np.float32)
        w1 = (rng.standard_normal((K1, Cc, 1, 1)) * np.sqrt(2.0 / Cc)).astype(np.float32)
        b1 = (rng.standard_normal(K1) * 0.5).astype(np.float32)
        w2 = (rng.standard_normal((Cc, K1, 1, 1)) * np.sqrt(2.0 / K1)).astype(np.float32)
        b2 = (rng.standard_normal(Cc) * 0.5).astype(np.float32)
        s_x, s_in, s_mid, s_res, s_sum, s_out = 0.023 + 0.001 * k, 0.02, 0.05, 0.043 + 0.002 * k, 0.06, 0.031
        c = 1.0 / s_sum
        odt2 = O.U8 if k % 2 == 0 else O.S8          # the next block's 3x3 input: both kinds
        relu2 = 1 if odt2 == O.U8 else 0
        ws0 = O.weight_scales(w0)
        bp0, sc0 = O.conv_i8_prepare(ws0, b0, s_x, s_in, idt, O.U8)
        t0 = O.conv_i8(cur_x, O.quant_weights(w0, ws0), bp0, sc0, O.U8, 1, (1, 1))
        ws1 = O.weight_scales(w1)
        bp1, sc1 = O.conv_i8_prepare(ws1, b1, s_in, s_mid, O.U8, O.S8)
        t1 = O.conv_i8(t0, O.quant_weights(w1, ws1), bp1, sc1, O.S8, 0)
        want1 = O.eltwise_i8(t1, cur_res, s_mid, s_res, c, c, True)
        ws2 = O.weight_scales(w2)
        bp2, sc2 = O.conv_i8_prepare(ws2, b2, s_sum, s_out, O.S8, odt2)
        want2 = O.conv_i8(want1, O.quant_weights(w2, ws2), bp2, sc2, odt2, relu2)
        c0 = S.SaberConv2D(int8=True).init((N, Cc, H, Wd), S.ConvParam(w0, b0, 1, (1, 1), (1, 1), (1, 1), True), idt, O.U8, s_x, s_in)
        pa = S.ConvParam(w1, b1, 1, (0, 0), (1, 1), (1, 1), False)
        pa.res_mode, pa.res_relu, pa.sum_scale, pa.coeff, pa.scale_res = L.RES_ELTWISE, True, 1.0, (c, c), s_res
        ca = S.SaberConv2D(int8=True).init((N, Cc, H, Wd), pa, O.U8, O.S8, s_in, s_mid)
        cb = S.SaberConv2D(int8=True).init((N, K1, H, Wd), S.ConvParam(w2, b2, 1, (0, 0), (1, 1), (1, 1), bool(relu2)), O.S8, odt2, s_sum, s_out)
        ops.append((c0, ca, cb))
        wants.append((want1, want2))
        cur_x, cur_res, idt = want2, want1, odt2
    return x, res, ops, wants


@pytest.mark.parametrize("shape", [(256, 8, 14, 14, 5), (256, 3, 14, 14, 3), (256, 2, 7, 9, 2), (256, 8, 14, 14, 1),
                                   (128, 8, 28, 28, 3), (128, 2, 9, 21, 2), (128, 1, 5, 13, 4), (128, 3, 7, 50, 2)])
def test_chain_stage_equals_the_chains_and_oracle(shape):
    """saber_hip_conv2d_stage_create: a RUN of res4 (C = 256: four cooperating workgroups per tile) or res3 (C = 128: one workgroup
    per tile, 1 / 2 / 4 column tiles) block chains in one persistent launch (conv_stage_coop.hip; an image per XCD, XCD-local edge
    barriers between blocks) - every block's two outputs bit for bit the oracle's and the chain launches', launch after launch (the
    arrival counters are never reset)."""
    Cc, N, H, Wd, nblk = shape
    rng = np.random.default_rng(4100 + N + H + nblk + Cc)
    x, res, ops, wants = _res4_blocks(rng, N, H, Wd, nblk, Cc=Cc)
    chains = [S.SaberConvChain(ca, cb, conv3x3=c0) for c0, ca, cb in ops]
    y1 = [ca.new_output() for _, ca, _ in ops]
    y2 = [cb.new_output() for _, _, cb in ops]
    cx, cr = dev(x), dev(res)
    for k, ch in enumerate(chains):                  # the chains one by one (their default single-workgroup form)
        ch.dispatch(cx, cr, y1[k], y2[k])
        assert np.array_equal(host(y1[k]), wants[k][0]) and np.array_equal(host(y2[k]), wants[k][1]), ("chain", k)
        cx, cr = y2[k], y1[k]
    stage = S.SaberChainStage(chains)
    for rep in range(3):
        for t in y1 + y2:
            t.fill_(77)
        stage.dispatch(dev(x), dev(res), y1, y2)
        for k in range(nblk):
            assert np.array_equal(host(y1[k]), wants[k][0]), ("stage y1", k, rep)
            assert np.array_equal(host(y2[k]), wants[k][1]), ("stage y2", k, rep)


def test_chain_stage_rejects_what_it_cannot_run():
    rng = np.random.default_rng(5)
    x, res, ops, wants = _res4_blocks(rng, 9, 14, 14, 2)          # batch 9: an image per XCD needs <= 8
    chains = [S.SaberConvChain(ca, cb, conv3x3=c0) for c0, ca, cb in ops]
    with pytest.raises(RuntimeError):
        S.SaberChainStage(chains)
    x, res, ops, wants = _res4_blocks(rng, 2, 6, 40, 2, Cc=128)   # width 40: three column tiles (arrivals per edge not a power of two)
    chains = [S.SaberConvChain(ca, cb, conv3x3=c0) for c0, ca, cb in ops]
    with pytest.raises(RuntimeError):
        S.SaberChainStage(chains)
    x, res, ops, wants = _res4_blocks(rng, 2, 6, 14, 1, Cc=128)   # C = 128: a stage is at least two blocks
    chains = [S.SaberConvChain(ca, cb, conv3x3=c0) for c0, ca, cb in ops]
    with pytest.raises(RuntimeError):
        S.SaberChainStage(chains)


def test_conv1x1_chain_rejects_other_shapes():
    rng = np.random.default_rng(3)
    w1 = (rng.standard_normal((128, 32, 1, 1)) * 0.2).astype(np.float32)
    w2 = (rng.standard_normal((32, 128, 1, 1)) * 0.2).astype(np.float32)
    pa = S.ConvParam(w1, None, 1, (0, 0), (1, 1), (1, 1), False)
    pa.res_mode, pa.res_relu, pa.sum_scale, pa.coeff, pa.scale_res = L.RES_ELTWISE, True, 1.0, (20.0, 20.0), 0.05
    ca = S.SaberConv2D(int8=True).init((1, 32, 8, 8), pa, O.U8, O.S8, 0.02, 0.05)
    cb = S.SaberConv2D(int8=True).init((1, 128, 8, 8), S.ConvParam(w2, None, 1, (0, 0), (1, 1), (1, 1), True), O.S8, O.U8,
                                       0.05, 0.03)
    with pytest.raises(L.SaberHipError):
        S.SaberConvChain(ca, cb)          # C = 32 has no chain kernel
    w1 = (rng.standard_normal((256, 64, 1, 1)) * 0.2).astype(np.float32)
    plain = S.SaberConv2D(int8=True).init((1, 64, 8, 8), S.ConvParam(w1, None, 1, (0, 0), (1, 1), (1, 1), False), O.U8,
                                          O.S8, 0.02, 0.05)
    w2 = (rng.standard_normal((64, 256, 1, 1)) * 0.2).astype(np.float32)
    cb = S.SaberConv2D(int8=True).init((1, 256, 8, 8), S.ConvParam(w2, None, 1, (0, 0), (1, 1), (1, 1), True), O.S8, O.U8,
                                       0.05, 0.03)
    with pytest.raises(L.SaberHipError):
        S.SaberConvChain(plain, cb)       # the first conv has no fused eltwise


PAIR_CASES = [
    # N, H, W, C, K1, K2, k, pad, stride
    (2, 14, 14, 64, 256, 64, 1, 0, 1),      # res2a: branch1 + branch2a
    (2, 14, 14, 256, 512, 128, 1, 0, 2),    # res3a (stride 2)
    (1, 9, 7, 128, 128, 48, 1, 0, 2),       # K2 not a tile multiple, odd spatial dims
    (1, 6, 6, 32, 128, 16, 3, 1, 1),        # 3x3 siblings
]


@pytest.mark.parametrize("case", PAIR_CASES)
@pytest.mark.parametrize("idt", [O.U8, O.S8])
def test_conv_i8_sibling_pair_equals_two_ops(case, idt):
    """saber_hip_conv2d_create_pair: one launch, both outputs bit-identical to the oracle (= to the two
    separate Saber ops of the reference op list), for every tile / staging variant."""
    N, H, W, C, K1, K2, k, pad, stride = case
    rng = np.random.default_rng(abs(hash((case, idt))) % 2**31)
    x = (rng.integers(0, 256, (N, H, W, C)).astype(np.uint8) if idt == O.U8
         else rng.integers(-128, 128, (N, H, W, C)).astype(np.int8))
    in_scale = 0.013
    convs, wants = [], []
    for K, odt, relu, out_scale in ((K1, O.S8, 0, 0.05), (K2, O.U8, 1, 0.031)):
        w = (rng.standard_normal((K, C, k, k)) * np.sqrt(2.0 / (C * k * k))).astype(np.float32)
        b = (rng.standard_normal(K) * 0.5).astype(np.float32)
        ws = O.weight_scales(w)
        bp, sc = O.conv_i8_prepare(ws, b, in_scale, out_scale, idt, odt)
        wants.append(O.conv_i8(x, O.quant_weights(w, ws), bp, sc, odt, relu, (pad, pad), (stride, stride)))
        p = S.ConvParam(w, b, 1, (pad, pad), (stride, stride), (1, 1), bool(relu))
        convs.append(S.SaberConv2D(True).init((N, C, H, W), p, idt, odt, in_scale, out_scale))
    pair = S.SaberConvPair(convs[0], convs[1])
    assert pair.algo().startswith("pair_igemm_i8")
    xd = dev(x)
    variants = [None] + [t | (ks << 8) | (1 << 16) for t in range(6) for ks in (1, 2, 4)] + \
               [t | (4 << 8) | (2 << 16) for t in range(6)] + [t | (4 << 8) | (3 << 16) for t in range(3)] + \
               [0 | (4 << 8) | (4 << 16)]
    for v in variants:
        if v is not None:
            pair.set_tile(v)
        ya, yb = convs[0].new_output(), convs[1].new_output()
        ya.fill_(77)
        yb.fill_(77)
        pair.dispatch(xd, ya, yb)
        assert np.array_equal(host(ya), wants[0]), (pair.algo(), "first")
        assert np.array_equal(host(yb), wants[1]), (pair.algo(), "second")
    # the parents stay usable on their own
    y0 = convs[0].new_output()
    convs[0].dispatch(xd, y0)
    assert np.array_equal(host(y0), wants[0])
    pair.autotune(xd, ya, yb, iters=2)
    pair.dispatch(xd, ya, yb)
    assert np.array_equal(host(ya), wants[0]) and np.array_equal(host(yb), wants[1]), pair.algo()


@pytest.mark.parametrize("case", [(2, 14, 14, 64, 256, 64, 1, 0, 1), (1, 9, 7, 128, 128, 48, 1, 0, 2),
                                  (1, 6, 6, 32, 128, 16, 3, 1, 1)])
def test_conv_f32_sibling_pair_equals_two_ops(case):
    """FP32 sibling pair: both outputs bit-identical to dispatching the two FP32 convs separately (same reduction
    order), and within 1e-4 of the oracle."""
    N, H, W, C, K1, K2, k, pad, stride = case
    rng = np.random.default_rng(abs(hash(case)) % 2**31)
    x = rng.standard_normal((N, H, W, C)).astype(np.float32)
    convs, wants = [], []
    for K, relu in ((K1, False), (K2, True)):
        w = (rng.standard_normal((K, C, k, k)) * np.sqrt(2.0 / (C * k * k))).astype(np.float32)
        b = (rng.standard_normal(K) * 0.5).astype(np.float32)
        wants.append(O.conv_f32_nchw(np.ascontiguousarray(x.transpose(0, 3, 1, 2)), w, b, relu, (pad, pad),
                                     (stride, stride)).transpose(0, 2, 3, 1))
        p = S.ConvParam(w, b, 1, (pad, pad), (stride, stride), (1, 1), relu)
        convs.append(S.SaberConv2D(False).init((N, C, H, W), p, L.F32, L.F32, in_layout=L.NHWC, out_layout=L.NHWC))
    xd = dev(x)
    sep = []
    for c in convs:
        y = c.new_output()
        c.dispatch(xd, y)
        sep.append(host(y).copy())
    pair = S.SaberConvPair(convs[0], convs[1])
    assert pair.algo().startswith("pair_igemm_f32")
    for v in [None, 0 | (1 << 8) | (1 << 16), 2 | (2 << 8) | (1 << 16), 3 | (4 << 8) | (1 << 16), 5 | (1 << 8) | (1 << 16),
              2 | (4 << 8) | (2 << 16), 1 | (4 << 8) | (3 << 16), 0 | (4 << 8) | (4 << 16)]:
        if v is not None:
            pair.set_tile(v)
            for c in convs:
                c.set_tile(v)       # same tile -> same reduction order -> identical bits
                y = c.new_output()
        ya, yb = convs[0].new_output(), convs[1].new_output()
        ya.fill_(7.0)
        yb.fill_(7.0)
        pair.dispatch(xd, ya, yb)
        if v is not None:
            for i, c in enumerate(convs):
                y = c.new_output()
                c.dispatch(xd, y)
                sep[i] = host(y).copy()
        for got, ref2, want in ((host(ya), sep[0], wants[0]), (host(yb), sep[1], wants[1])):
            assert np.array_equal(got, ref2), pair.algo()
            assert np.abs(got - want).max() <= FP32_RTOL * np.abs(want).max(), pair.algo()


def test_full_size_fused_ops_equal_their_unfused_gpu_forms():
    """Size-independent properties at BASELINE.json's full batch-8 sizes (the oracle would take minutes there): every
    fused executor op must reproduce, byte for byte, the separate ops it replaces when both run on the GPU —
    sibling pair vs two convs (res3a: 8x56x56x256 -> 512 / 128, stride 2), SaberConv2DPooling vs conv then pooling
    (conv1 + pool1 on 8x3x224x224), fused pool5 quantise vs pool then quantise."""
    rng = np.random.default_rng(2026)
    # --- sibling pair, res3a geometry
    N, H, C, K1, K2 = 8, 56, 256, 512, 128
    x = dev(rng.integers(0, 256, (N, H, H, C)).astype(np.uint8))
    convs = []
    for K, odt, relu, osc in ((K1, O.S8, False, 0.05), (K2, O.U8, True, 0.03)):
        w = (rng.standard_normal((K, C, 1, 1)) * np.sqrt(2.0 / C)).astype(np.float32)
        b = (rng.standard_normal(K) * 0.5).astype(np.float32)
        p = S.ConvParam(w, b, 1, (0, 0), (2, 2), (1, 1), relu)
        convs.append(S.SaberConv2D(True).init((N, C, H, H), p, O.U8, odt, 0.013, osc))
    sep = [c.dispatch(x, c.new_output()) for c in convs]
    pair = S.SaberConvPair(convs[0], convs[1])
    ya, yb = convs[0].new_output(), convs[1].new_output()
    pair.autotune(x, ya, yb, iters=2)
    ya.zero_(), yb.zero_()
    pair.dispatch(x, ya, yb)
    torch.cuda.synchronize()
    assert torch.equal(ya, sep[0]) and torch.equal(yb, sep[1]), pair.algo()
    # --- conv1 + pool1
    xf = dev(rng.uniform(-1, 1, (8, 3, 224, 224)).astype(np.float32))
    w = (rng.standard_normal((64, 3, 7, 7)) * 0.1).astype(np.float32)
    b = (rng.standard_normal(64) * 0.3).astype(np.float32)
    p = S.ConvParam(w, b, 1, (3, 3), (2, 2), (1, 1), True)
    conv = S.SaberConv2D(True).init((8, 3, 224, 224), p, L.F32, O.U8, 1 / 127.0, 0.02, in_layout=L.NCHW)
    mid = conv.dispatch(xf, conv.new_output())
    want = S.pooling_i8(mid, (3, 3), (2, 2), (0, 0), L.POOL_MAX)
    cp = S.SaberConv2DPooling().init((8, 3, 224, 224), p, L.POOL_MAX, (3, 3), (2, 2), (0, 0), L.F32, O.U8, 1 / 127.0, 0.02,
                                     in_layout=L.NCHW)
    assert cp.fused
    got = cp.dispatch(xf, cp.new_output())
    torch.cuda.synchronize()
    assert got.shape == want.shape and torch.equal(got, want)
    # --- pool5 + quantise
    x5 = dev(rng.integers(-128, 128, (8, 7, 7, 2048)).astype(np.int8))
    y = S.pooling_f32_from_i8(x5, 0.06, None, None, None, 1, global_pooling=True)
    y2, yq = S.pooling_f32_from_i8(x5, 0.06, None, None, None, 1, global_pooling=True, q_scale=0.011)
    torch.cuda.synchronize()
    assert torch.equal(y, y2) and np.array_equal(host(yq), O.quant_flat_s8(host(y), 0.011))


def test_conv_i8_sibling_pair_rejects_mismatches():
    rng = np.random.default_rng(3)
    def mk(K, C=32, k=1, stride=1, odt=O.S8):
        w = rng.standard_normal((K, C, k, k)).astype(np.float32)
        p = S.ConvParam(w, None, 1, (0, 0), (stride, stride), (1, 1), odt == O.U8)
        return S.SaberConv2D(True).init((1, C, 8, 8), p, O.U8, odt, 0.02, 0.03)
    a = mk(128)
    with pytest.raises(L.SaberHipError):
        S.SaberConvPair(a, mk(64, stride=2))          # different geometry
    with pytest.raises(L.SaberHipError):
        S.SaberConvPair(mk(64), mk(64))               # first K not a multiple of 128
    with pytest.raises(L.SaberHipError):
        S.SaberConvPair(a, mk(24))                    # second K not a multiple of 16
    pair = S.SaberConvPair(a, mk(64, odt=O.U8))
    y = a.new_output()
    with pytest.raises(L.SaberHipError):              # a pair cannot go through the single-output entry point
        L.check(L.load().saber_hip_conv2d_run(pair.h, S._p(y), S._p(y), None, None, None))


def test_conv_i8_jit_sum_inplace():
    rng = np.random.default_rng(13)
    x = rng.integers(-128, 128, (1, 7, 7, 32)).astype(np.int8)
    w = (rng.standard_normal((32, 32, 3, 3)) * 0.1).astype(np.float32)
    prev = rng.integers(0, 200, (1, 7, 7, 32)).astype(np.uint8)
    ws = O.weight_scales(w)
    bp, sc = O.conv_i8_prepare(ws, None, 0.03, 0.04, O.S8, O.U8)
    for sum_scale in (1.0, 0.37):
        rp = O.Residual(O.RES_JIT_SUM, 0, sum_scale, O.U8, 0, 0, 0, 0)
        want = O.conv_i8(x, O.quant_weights(w, ws), None, sc, O.U8, 1, (1, 1), residual=rp, out_init=prev)
        got, conv = run_conv_i8(x, w, None, None, 0.03, 0.04, O.U8, 1, 1, 1, 1, 1,
                                res_param=(L.RES_SUM_INPLACE, False, sum_scale, (1.0, 1.0), 1.0), y_init=prev)
        assert np.array_equal(got, want), conv.algo()
    # the bytes already in y need not have the output's dtype (ConvParam::beta_type): s8 added into a u8 output and u8
    # into an s8 output, every kernel family that can carry the generic epilogue
    x3 = rng.integers(0, 256, (2, 14, 14, 64)).astype(np.uint8)
    w3 = (rng.standard_normal((64, 64, 3, 3)) * 0.06).astype(np.float32)
    b3 = (rng.standard_normal(64) * 0.4).astype(np.float32)
    ws3 = O.weight_scales(w3)
    for odt, rdt, relu in ((O.U8, O.S8, 1), (O.S8, O.U8, 0)):
        prev = (rng.integers(-128, 128, (2, 14, 14, 64)).astype(np.int8) if rdt == O.S8
                else rng.integers(0, 256, (2, 14, 14, 64)).astype(np.uint8))
        bp3, sc3 = O.conv_i8_prepare(ws3, b3, 0.02, 0.05, O.U8, odt)
        rp = O.Residual(O.RES_JIT_SUM, 0, 0.61, rdt, 0, 0, 0, 0)
        prev_as_out = prev.view(np.uint8 if odt == O.U8 else np.int8)
        want = O.conv_i8(x3, O.quant_weights(w3, ws3), bp3, sc3, odt, relu, (1, 1), residual=rp, out_init=prev_as_out)
        for tile in (None, 2 | (1 << 8) | (1 << 16), 1 | (4 << 8) | (3 << 16), 6 << 16, 7 | (1 << 8) | (9 << 16)):
            N, H, W_, Cc = x3.shape
            p = S.ConvParam(w3, b3, 1, (1, 1), (1, 1), (1, 1), bool(relu))
            p.res_mode, p.res_relu, p.sum_scale, p.res_dtype = L.RES_SUM_INPLACE, False, 0.61, rdt
            conv = S.SaberConv2D(int8=True).init((N, Cc, H, W_), p, O.U8, odt, 0.02, 0.05)
            if tile is not None:
                conv.set_tile(tile)
            y = conv.new_output()
            y.copy_(dev(prev_as_out))
            conv.dispatch(dev(x3), y)
            assert np.array_equal(host(y), want), (conv.algo(), odt, rdt)
    with pytest.raises(L.SaberHipError):   # an f32 residual under an 8-bit output has no in-place meaning
        p = S.ConvParam(w3, b3, 1, (1, 1), (1, 1), (1, 1), True)
        p.res_mode, p.res_dtype = L.RES_SUM_INPLACE, L.F32
        S.SaberConv2D(int8=True).init((2, 64, 14, 14), p, O.U8, O.U8, 0.02, 0.05)


def test_quant_dequant_golden():
    g = load("quant_dequant")
    s = float(g["scale"])
    x = dev(g["x"])
    assert np.array_equal(host(S.quantize_nchw_to_nhwc(x, s, L.S8)), g["q_s8"])
    assert np.array_equal(host(S.quantize_nchw_to_nhwc(x, s, L.U8)), g["q_u8"])
    assert np.array_equal(host(S.dequantize_nhwc_to_nchw(dev(g["q_s8"]), s)), g["deq_s8"])
    assert np.array_equal(host(S.dequantize_nhwc_to_nchw(dev(g["q_u8"]), s)), g["deq_u8"])
    # channel padding (first layer: C=3 -> 4) writes zeros in the pad lane
    xp = np.random.default_rng(1).uniform(-1, 1, (2, 3, 5, 6)).astype(np.float32)
    q = host(S.quantize_nchw_to_nhwc(dev(xp), 0.01, L.S8, c_pad=4))
    assert np.array_equal(q[..., :3], O.quant_nchw_to_nhwc(xp, 0.01, O.S8)) and not q[..., 3].any()


def test_eltwise_golden_and_ragged():
    g = load("eltwise")
    sa, sb, c = float(g["sa"]), float(g["sb"]), float(g["c"])
    assert np.array_equal(host(S.eltwise_sum(dev(g["a"]), dev(g["b"]), (c, c), True, sa, sb)), g["y_relu"])
    assert np.array_equal(host(S.eltwise_sum(dev(g["a"]), dev(g["b"]), (1, 1), False, sa, sb)), g["y_lin"])
    assert np.array_equal(host(S.eltwise_sum(dev(g["fa"]), dev(g["fb"]), (1, 1), True)), g["yf"])
    rng = np.random.default_rng(2)
    a = rng.integers(-128, 128, 1003).astype(np.int8)   # not a multiple of the 16-byte vector
    b = rng.integers(-128, 128, 1003).astype(np.int8)
    assert np.array_equal(host(S.eltwise_sum(dev(a), dev(b), (7.5, 3.25), True, 0.1, 0.2)),
                          O.eltwise_i8(a, b, 0.1, 0.2, 7.5, 3.25, True))


@pytest.mark.parametrize("name", conv_f32_fixtures())
def test_conv_f32_golden(name):
    g = load(name)
    N, C, H, W, K, k, pad, stride = [int(v) for v in g["spec"]]
    p = S.ConvParam(g["w"], g["bias"], 1, (pad, pad), (stride, stride), (1, 1), True)
    conv = S.SaberConv2D(int8=False).init((N, C, H, W), p, L.F32, L.F32)
    y = conv.new_output()
    conv.dispatch(dev(g["x"]), y)
    err = np.abs(host(y) - g["y"]).max() / np.abs(g["y"]).max()
    assert err <= FP32_RTOL, (conv.algo(), err)


def test_conv_f32_residual_golden():
    g = load("conv_f32_1x1_residual_mkl")   # produced by SaberConv1X1 (MKL sgemm, beta = 1)
    p = S.ConvParam(g["w"], g["bias"], 1, (0, 0), (1, 1), (1, 1), False)
    p.res_mode, p.res_relu = L.RES_SUM_INPLACE, True
    conv = S.SaberConv2D(int8=False).init(g["x"].shape, p, L.F32, L.F32)
    y = dev(g["res"])
    conv.dispatch(dev(g["x"]), y)
    err = np.abs(host(y) - g["y"]).max() / np.abs(g["y"]).max()
    assert err <= FP32_RTOL, (conv.algo(), err)


@pytest.mark.parametrize("case", [(2, 20, 9, 9, 24, 3, 1, 1, 1), (1, 8, 12, 12, 8, 3, 1, 1, 2),
                                  (1, 64, 14, 14, 256, 1, 0, 1, 1), (2, 16, 15, 15, 32, 3, 1, 2, 1)])
def test_conv_f32_sweep_vs_oracle(case):
    N, C, H, W, K, k, pad, stride, group = case
    rng = np.random.default_rng(21)
    x = rng.standard_normal((N, C, H, W)).astype(np.float32)
    w = (rng.standard_normal((K, C // group, k, k)) * 0.1).astype(np.float32)
    b = rng.standard_normal(K).astype(np.float32)
    want = O.conv_f32_nchw(x, w, b, True, (pad, pad), (stride, stride), (1, 1), group)
    p = S.ConvParam(w, b, group, (pad, pad), (stride, stride), (1, 1), True)
    conv = S.SaberConv2D(False).init(x.shape, p, L.F32, L.F32)
    y = conv.new_output()
    conv.dispatch(dev(x), y)
    err = np.abs(host(y) - want).max() / np.abs(want).max()
    assert err <= FP32_RTOL, (conv.algo(), err)


@pytest.mark.parametrize("dt", [O.S8, O.U8])
def test_pooling_i8_vs_oracle(dt):
    rng = np.random.default_rng(31)
    mk = (lambda s: rng.integers(0, 256, s).astype(np.uint8)) if dt == O.U8 else \
        (lambda s: rng.integers(-128, 128, s).astype(np.int8))
    x = mk((2, 112, 112, 64)[:1] + (30, 30, 64))
    for (win, st, pad, pt) in [((3, 3), (2, 2), (0, 0), 0), ((3, 3), (2, 2), (1, 1), 0), ((2, 2), (2, 2), (0, 0), 1),
                               ((3, 3), (2, 2), (1, 1), 2), ((3, 3), (1, 1), (1, 1), 1)]:
        want = O.pool_i8_nhwc(x, win, st, pad, pt)
        got = host(S.pooling_i8(dev(x), win, st, pad, pt))
        assert np.array_equal(got, want), (win, st, pad, pt)
    x7 = mk((3, 7, 7, 2048))
    assert np.array_equal(host(S.pooling_i8(dev(x7), None, None, None, 1, global_pooling=True)),
                          O.pool_i8_nhwc(x7, None, None, None, 1, global_pool=True))
    assert np.array_equal(host(S.pooling_i8(dev(x7), None, None, None, 1, out_dtype=L.F32, global_pooling=True)),
                          O.pool_i8_nhwc(x7, None, None, None, 1, out_dtype=O.F32, global_pool=True))
    xo = mk((1, 9, 9, 10))  # channel count not a multiple of 4
    assert np.array_equal(host(S.pooling_i8(dev(xo), (3, 3), (2, 2), (0, 0), 0)),
                          O.pool_i8_nhwc(xo, (3, 3), (2, 2), (0, 0), 0))


def test_pooling_f32_vs_oracle():
    rng = np.random.default_rng(32)
    x = rng.standard_normal((2, 16, 13, 13)).astype(np.float32)
    for (win, st, pad, pt) in [((3, 3), (2, 2), (0, 0), 0), ((3, 3), (2, 2), (1, 1), 1), ((2, 2), (2, 2), (0, 0), 2)]:
        want = O.pool_f32_nchw(x, win, st, pad, pt)
        got = host(S.pooling_f32(dev(x), win, st, pad, pt))
        assert np.array_equal(got, want), (win, st, pad, pt)
    want = O.pool_f32_nchw(x, None, None, None, 1, global_pool=True)
    assert np.array_equal(host(S.pooling_f32(dev(x), None, None, None, 1, global_pooling=True)), want)
    # NHWC: the float4-vectorised kernel (c % 4 == 0) and the scalar one (c = 6) — same bits as the NCHW oracle
    for c in (16, 6):
        xc = rng.standard_normal((2, c, 11, 14)).astype(np.float32)
        xh = np.ascontiguousarray(xc.transpose(0, 2, 3, 1))
        for (win, st, pad, pt) in [((3, 3), (2, 2), (0, 0), 0), ((3, 3), (2, 2), (1, 1), 1), ((2, 2), (2, 2), (0, 0), 2),
                                   ((3, 3), (1, 1), (1, 1), 0)]:
            want = O.pool_f32_nchw(xc, win, st, pad, pt).transpose(0, 2, 3, 1)
            got = host(S.pooling_f32(dev(xh), win, st, pad, pt, layout=L.NHWC))
            assert np.array_equal(got, want), (c, win, st, pad, pt)
    # NHWC global pooling (ResNet pool5, <= 64 pixels): the all-loads-in-flight kernel keeps the reference's summation order
    for (c, hh, ww, pt) in ((256, 7, 7, 1), (6, 5, 8, 2), (32, 3, 3, 0), (8, 8, 8, 1)):
        xc = rng.standard_normal((3, c, hh, ww)).astype(np.float32)
        xh = np.ascontiguousarray(xc.transpose(0, 2, 3, 1))
        want = O.pool_f32_nchw(xc, None, None, None, pt, global_pool=True).transpose(0, 2, 3, 1)
        got = host(S.pooling_f32(dev(xh), None, None, None, pt, global_pooling=True, layout=L.NHWC))
        assert np.array_equal(got, want), (c, hh, ww, pt)


def test_pooling_f32_from_i8_equals_dequant_then_pool():
    rng = np.random.default_rng(33)
    for dt, mk in ((O.S8, lambda s: rng.integers(-128, 128, s).astype(np.int8)),
                   (O.U8, lambda s: rng.integers(0, 256, s).astype(np.uint8))):
        x = mk((3, 7, 7, 2048))
        want = O.pool_f32_nchw(O.dequant_nhwc_to_nchw(x, 0.37), None, None, None, 1, global_pool=True)
        got = host(S.pooling_f32_from_i8(dev(x), 0.37, None, None, None, 1, global_pooling=True))
        assert np.array_equal(got, want)
        x = mk((2, 13, 13, 24))
        want = O.pool_f32_nchw(O.dequant_nhwc_to_nchw(x, 0.05), (3, 3), (2, 2), (1, 1), 0)
        assert np.array_equal(host(S.pooling_f32_from_i8(dev(x), 0.05, (3, 3), (2, 2), (1, 1), 0)), want)
        # fused quantise-on-entry of the next INT8 op: same f32 result + its s8 quantisation (both kernel paths)
        y, yq = S.pooling_f32_from_i8(dev(x), 0.05, (3, 3), (2, 2), (1, 1), 0, q_scale=0.011)
        assert np.array_equal(host(y), want) and np.array_equal(host(yq), O.quant_flat_s8(want, 0.011))
        x = mk((3, 7, 7, 2048))
        want = O.pool_f32_nchw(O.dequant_nhwc_to_nchw(x, 0.37), None, None, None, 1, global_pool=True)
        for qs in (0.2, 0.01):   # the small scale saturates
            y, yq = S.pooling_f32_from_i8(dev(x), 0.37, None, None, None, 1, global_pooling=True, q_scale=qs)
            assert np.array_equal(host(y), want) and np.array_equal(host(yq), O.quant_flat_s8(want, qs))


def test_fc_i8_golden():
    """INT8 fc (f32 input quantised on entry) against the fixture produced by the reference's PackedMKLInt8Gemm."""
    g = load("fc_i8_f32in")
    w = g["w"].astype(np.float32)
    N, K = w.shape
    M = g["x"].shape[0]
    fc = S.SaberFc(True).init(M, N, K, w, g["bias"], L.F32, float(g["in_scale"]))
    y = torch.empty((M, N), dtype=torch.float32, device="cuda")
    assert np.array_equal(host(fc.dispatch(dev(g["x"]), y)), g["y"])


def test_fc_vs_oracle():
    rng = np.random.default_rng(41)
    M, N, K = 8, 1000, 2048
    w = (rng.standard_normal((N, K)) * 0.02).astype(np.float32)
    b = rng.standard_normal(N).astype(np.float32)
    ws = O.weight_scales(w)
    wq = O.quant_weights(w, ws)
    # INT8 fc, f32 input: quantise on entry (PackedMKLInt8Gemm), f32 out — bit exact
    xf = rng.standard_normal((M, K)).astype(np.float32)
    in_scale = float(np.abs(xf).max() / 127)
    want = O.fc_i8(O.quant_flat_s8(xf, in_scale), wq, ws, in_scale, b)
    fc = S.SaberFc(True).init(M, N, K, w, b, L.F32, in_scale)
    assert fc.algo() == "fc_i8_small_16xk4", fc.algo()   # STATIC choice for <= 16 rows
    y = torch.empty((M, N), dtype=torch.float32, device="cuda")
    assert np.array_equal(host(fc.dispatch(dev(xf), y)), want)
    fc.set_tile(0 | (4 << 8) | (1 << 16))   # the implicit-GEMM kernel computes the same bits
    y.zero_()
    assert fc.algo().startswith("igemm_i8") and np.array_equal(host(fc.dispatch(dev(xf), y)), want)
    fc.set_tile(10 << 16)
    y.zero_()   # the same op fed the already-quantised input (producer fused the quantise-on-entry)
    assert np.array_equal(host(fc.dispatch_q(dev(O.quant_flat_s8(xf, in_scale)), y)), want)
    # s8 input
    xs = rng.integers(-128, 128, (M, K)).astype(np.int8)
    fc = S.SaberFc(True).init(M, N, K, wq, b, L.S8, 0.031, w_scale=ws)
    assert np.array_equal(host(fc.dispatch(dev(xs), y)), O.fc_i8(xs, wq, ws, 0.031, b))
    # u8 input (VenderFc<X86,AK_INT8> u8 path: int bias, scale*(acc+bias))
    xu = rng.integers(0, 256, (M, K)).astype(np.uint8)
    fc = S.SaberFc(True).init(M, N, K, wq, b, L.U8, 0.031, 0.5, w_scale=ws)
    assert np.array_equal(host(fc.dispatch(dev(xu), y)), O.fc_i8(xu, wq, ws, 0.031, b, 0.5))
    # FP32 fc, both weight layouts
    want = O.fc_f32(xf, w, b)
    fc = S.SaberFc(False).init(M, N, K, w, b, L.F32)
    assert np.abs(host(fc.dispatch(dev(xf), y)) - want).max() <= FP32_RTOL * np.abs(want).max()
    fc = S.SaberFc(False).init(M, N, K, np.ascontiguousarray(w.T), b, L.F32, w_is_kn=True)
    assert np.abs(host(fc.dispatch(dev(xf), y)) - want).max() <= FP32_RTOL * np.abs(want).max()
    assert fc.algo().startswith("fc_f32_small")
    # ragged FP32 shapes through the small-batch kernel (k not a multiple of the 64-float wave stride, n not of 16 / 4)
    for (m2, n2, k2) in ((1, 10, 36), (16, 1000, 2048), (5, 33, 100), (3, 7, 4096)):
        w2 = (rng.standard_normal((n2, k2)) * 0.05).astype(np.float32)
        b2 = rng.standard_normal(n2).astype(np.float32)
        x2 = rng.standard_normal((m2, k2)).astype(np.float32)
        fc2 = S.SaberFc(False).init(m2, n2, k2, w2, b2, L.F32)
        y2 = torch.empty((m2, n2), dtype=torch.float32, device="cuda")
        want2 = O.fc_f32(x2, w2, b2)
        assert fc2.algo().startswith("fc_f32_small"), fc2.algo()
        assert np.abs(host(fc2.dispatch(dev(x2), y2)) - want2).max() <= FP32_RTOL * np.abs(want2).max(), (m2, n2, k2)


@pytest.mark.parametrize("shape", [(1, 1000, 2048), (16, 1000, 2048), (5, 24, 4096), (3, 1000, 528), (8, 50, 16),
                                   (17, 64, 2048), (4, 64, 4112)])
@pytest.mark.parametrize("idt", [O.S8, O.U8])
def test_fc_small_batch_kernel(shape, idt):
    """fc_small.hip over batch rows 1..16, ragged n, reduction lengths that leave partial / empty k-steps; shapes outside
    its limits (m > 16, k > 4096) keep the implicit-GEMM kernel. Both must equal the oracle bit for bit."""
    M, N, K = shape
    rng = np.random.default_rng(abs(hash((shape, idt))) % 2**31)
    wq = rng.integers(-127, 128, (N, K)).astype(np.int8)
    ws = (rng.random(N).astype(np.float32) * 0.01 + 0.001)
    b = rng.standard_normal(N).astype(np.float32)
    x = (rng.integers(0, 256, (M, K)).astype(np.uint8) if idt == O.U8 else rng.integers(-128, 128, (M, K)).astype(np.int8))
    fc = S.SaberFc(True).init(M, N, K, wq, b, idt, 0.031, 0.5, w_scale=ws)
    small = M <= 16 and K <= 4096
    assert (fc.algo() == "fc_i8_small_16xk4") == small, (fc.algo(), shape)
    want = O.fc_i8(x, wq, ws, 0.031, b, 0.5) if idt == O.U8 else O.fc_i8(x, wq, ws, 0.031, b)
    y = torch.full((M, N), -7.0, dtype=torch.float32, device="cuda")
    assert np.array_equal(host(fc.dispatch(dev(x), y)), want)
    if small:
        fc.set_tile(0 | (4 << 8) | (1 << 16))
        y.fill_(-7.0)
        assert fc.algo().startswith("igemm_i8") and np.array_equal(host(fc.dispatch(dev(x), y)), want)
    else:
        with pytest.raises(L.SaberHipError):
            fc.set_tile(10 << 16)


@pytest.mark.parametrize("case", [(2, 16, 12, 12, 32, 3, 1), (1, 64, 28, 20, 48, 3, 1), (3, 8, 6, 10, 20, 1, 0), (1, 4, 16, 16, 64, 3, 1)])
def test_conv_f32_fused_relu_maxpool2x2(case):
    """SaberConv2DPooling, FP32: conv + relu + 2x2 / stride-2 max pooling in one launch (pool-ordered GEMM columns, quad
    maximum in the epilogue) == the same conv followed by the pooling kernel BIT FOR BIT (same float values, a maximum has
    no rounding), for every tile / stage depth / staging, and within 1e-4 of the oracle's conv -> pool."""
    N, C, H, W, K, k, pad = case
    rng = np.random.default_rng(abs(hash(case)) % 2**31)
    x = rng.standard_normal((N, H, W, C)).astype(np.float32)          # NHWC on the device
    w = (rng.standard_normal((K, C, k, k)) * np.sqrt(2.0 / (C * k * k))).astype(np.float32)
    b = (rng.standard_normal(K) * 0.3).astype(np.float32)
    p = S.ConvParam(w, b, 1, (pad, pad), (1, 1), (1, 1), True)
    want = O.pool_f32_nchw(O.conv_f32_nchw(x.transpose(0, 3, 1, 2), w, b, True, (pad, pad)), (2, 2), (2, 2), (0, 0), 0)
    two = S.SaberConv2D(False).init((N, C, H, W), p, L.F32, L.F32, in_layout=L.NHWC, out_layout=L.NHWC)
    y2 = two.new_output()
    two.dispatch(dev(x), y2)
    unfused = host(S.pooling_f32(y2, (2, 2), (2, 2), (0, 0), 0, layout=L.NHWC))
    for var in (1, 2):
        for tile in range(len(L.TILES)):
            for ks in (1, 4):
                cp = S.SaberConv2DPooling(int8=False).init((N, C, H, W), p, 0, (2, 2), (2, 2), (0, 0), L.F32, L.F32)
                assert cp.fused and cp.out_hw == (H // 2 if pad or k == 1 else (H - 2) // 2, W // 2 if pad or k == 1 else (W - 2) // 2)
                cp.conv.set_tile(tile | (ks << 8) | (var << 16))
                y = cp.new_output()
                cp.dispatch(dev(x), y)
                got = host(y)
                assert cp.algo().endswith("+maxpool2x2"), cp.algo()
                assert np.array_equal(got, unfused), cp.algo()
    assert np.abs(got.transpose(0, 3, 1, 2) - want).max() <= FP32_RTOL * np.abs(want).max()
    # no fused kernel for other pooling geometries or un-relu'd convs: the two-launch structure is used
    cp = S.SaberConv2DPooling(int8=False).init((N, C, H, W), p, 0, (3, 3), (2, 2), (0, 0), L.F32, L.F32)
    assert not cp.fused
    y = cp.new_output()
    cp.dispatch(dev(x), y)
    assert np.array_equal(host(y), host(S.pooling_f32(y2, (3, 3), (2, 2), (0, 0), 0, layout=L.NHWC)))
    p0 = S.ConvParam(w, b, 1, (pad, pad), (1, 1), (1, 1), False)
    assert not S.SaberConv2DPooling(int8=False).init((N, C, H, W), p0, 0, (2, 2), (2, 2), (0, 0), L.F32, L.F32).fused


@pytest.mark.parametrize("case", [(2, 32, 12, 20, 32), (1, 64, 28, 36, 48), (2, 96, 6, 10, 128)])
@pytest.mark.parametrize("variant", [1, 2, 3, 4, 5])
def test_conv_f32_halo_kernel_fused_relu_maxpool2x2(case, variant):
    """SaberConv2DPooling FP32 on the LDS-halo bf16-plane kernel: a pooling window is two rows of one wave x a lane pair; the pooled
    tensor is within 1e-4 of the oracle's conv -> pool and EQUAL to max-pooling this kernel's own unpooled output (a maximum has no
    rounding)."""
    N, C, H, W, K = case
    rng = np.random.default_rng(N + C + H + K + variant)
    x = rng.standard_normal((N, H, W, C)).astype(np.float32)
    w = (rng.standard_normal((K, C, 3, 3)) * np.sqrt(2.0 / (C * 9))).astype(np.float32)
    b = (rng.standard_normal(K) * 0.3).astype(np.float32)
    p = S.ConvParam(w, b, 1, (1, 1), (1, 1), (1, 1), True)
    want = O.pool_f32_nchw(O.conv_f32_nchw(x.transpose(0, 3, 1, 2), w, b, True, (1, 1)), (2, 2), (2, 2), (0, 0), 0)
    two = S.SaberConv2D(False).init((N, C, H, W), p, L.F32, L.F32, in_layout=L.NHWC, out_layout=L.NHWC)
    two.set_tile(variant | (13 << 16))
    y2 = two.new_output()
    two.dispatch(dev(x), y2)
    unfused = host(S.pooling_f32(y2, (2, 2), (2, 2), (0, 0), 0, layout=L.NHWC))
    cp = S.SaberConv2DPooling(int8=False).init((N, C, H, W), p, 0, (2, 2), (2, 2), (0, 0), L.F32, L.F32)
    assert cp.fused
    cp.conv.set_tile(variant | (13 << 16))
    assert cp.algo().startswith("halo3x3_f32_bf16x3") and cp.algo().endswith("+maxpool2x2"), cp.algo()
    y = cp.new_output()
    y.fill_(-5.0)
    cp.dispatch(dev(x), y)
    got = host(y)
    assert np.array_equal(got, unfused), cp.algo()
    assert np.abs(got.transpose(0, 3, 1, 2) - want).max() <= FP32_RTOL * np.abs(want).max()


def test_conv_f32_leaky_relu():
    """ActivationParam::negative_slope of an Active_relu on the FP32 conv: "if (t < 0) t *= slope" after the bias
    (saber_im2col_conv.cpp:153-207, saber_conv_1x1.cpp:61-64). INT8 convs reject it (the x86 INT8 conv clamps to 0)."""
    rng = np.random.default_rng(71)
    for (N, C, H, W, K, k, pad, stride) in ((2, 16, 9, 11, 24, 3, 1, 1), (1, 32, 8, 8, 40, 1, 0, 2)):
        x = rng.standard_normal((N, C, H, W)).astype(np.float32)
        w = (rng.standard_normal((K, C, k, k)) * 0.2).astype(np.float32)
        b = rng.standard_normal(K).astype(np.float32)
        lin = O.conv_f32_nchw(x, w, b, False, (pad, pad), (stride, stride))
        want = np.where(lin < 0, lin * np.float32(0.1), lin).astype(np.float32)
        for layout in (L.NCHW, L.NHWC):
            p = S.ConvParam(w, b, 1, (pad, pad), (stride, stride), (1, 1), True)
            p.negative_slope = 0.1
            conv = S.SaberConv2D(False).init((N, C, H, W), p, L.F32, L.F32, in_layout=layout, out_layout=layout)
            y = conv.new_output()
            conv.dispatch(dev(x if layout == L.NCHW else np.ascontiguousarray(x.transpose(0, 2, 3, 1))), y)
            got = host(y) if layout == L.NCHW else host(y).transpose(0, 3, 1, 2)
            assert np.abs(got - want).max() <= FP32_RTOL * np.abs(want).max() and (got < 0).any()
    p = S.ConvParam(w, b, 1, (0, 0), (2, 2), (1, 1), True)
    p.negative_slope = 0.1
    with pytest.raises(L.SaberHipError):
        S.SaberConv2D(True).init((1, 32, 8, 8), p, L.S8, L.U8, 0.02, 0.05)


@pytest.mark.parametrize("ta,tb", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_gemm_f32_vs_oracle(ta, tb):
    rng = np.random.default_rng(51)
    M, N, K = 70, 130, 45   # ragged on purpose
    A = rng.standard_normal((K, M) if ta else (M, K)).astype(np.float32)
    B = rng.standard_normal((N, K) if tb else (K, N)).astype(np.float32)
    C0 = rng.standard_normal((M, N)).astype(np.float32)
    want = O.gemm_f32(A, B, M, N, K, ta, tb, 0.7, 0.3, C0)
    c = dev(C0)
    S.gemm(ta, tb, M, N, K, 0.7, dev(A), dev(B), 0.3, c)
    assert np.abs(host(c) - want).max() <= FP32_RTOL * np.abs(want).max()


@pytest.mark.parametrize("ta,tb", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_gemm_f32_plane_path_vs_oracle(ta, tb):
    """Gemm<MI355X, float, float> on the bf16-plane kernels (api_gemm.hip: device-side split of alpha * op(B)^T into three bf16 planes,
    the MODE 3 implicit-GEMM kernel, beta through the in-place sum epilogue): every transpose combination x ragged m / n (k % 8 == 0 is
    the path's condition; other k take the f32-MFMA kernel, test above) x beta in {0, 1, general}, within 1e-4 of the oracle on the
    max-norm AND element-wise with the mean magnitude as the floor; repeated calls (the plan cache) give the same bits."""
    rng = np.random.default_rng(52 + ta * 2 + tb)
    for (M, N, K), (alpha, beta) in (((333, 200, 264), (1.0, 0.0)), ((70, 1000, 2048), (0.7, 0.3)), ((512, 384, 512), (1.0, 1.0)),
                                     ((8, 4096, 25088 // 8), (1.0, 0.0)), ((3, 1000, 2048), (0.5, 0.25)), ((16, 515, 4100), (1.0, 1.0))):
        A = rng.standard_normal((K, M) if ta else (M, K)).astype(np.float32)
        B = rng.standard_normal((N, K) if tb else (K, N)).astype(np.float32)
        C0 = rng.standard_normal((M, N)).astype(np.float32)
        a64 = (A.T if ta else A).astype(np.float64)
        b64 = (B.T if tb else B).astype(np.float64)
        want = alpha * (a64 @ b64) + beta * C0
        got = None
        for rep in range(2):
            c = dev(C0)
            S.gemm(ta, tb, M, N, K, alpha, dev(A), dev(B), beta, c)
            g = host(c)
            assert got is None or np.array_equal(got, g)
            got = g
        d = np.abs(got - want)
        e_max = float(d.max() / np.abs(want).max())
        e_el = float((d / (np.abs(want) + np.abs(want).mean())).max())
        assert e_max <= FP32_RTOL and e_el <= FP32_RTOL, (M, N, K, e_max, e_el)
        ref32 = O.gemm_f32(A, B, M, N, K, ta, tb, alpha, beta, C0) if M * N * K <= 70 * 1000 * 2048 else None
        if ref32 is not None:
            assert np.abs(got - ref32).max() <= FP32_RTOL * np.abs(ref32).max()


def test_gemm_f32_b_changes_between_calls_and_streams_have_their_own_plans():
    """B is a raw device pointer: its planes are re-split on every call (a weight that changed is picked up); two streams get
    two plans (their scratch must not be shared)."""
    rng = np.random.default_rng(58)
    M = N = K = 256
    A = rng.standard_normal((M, K)).astype(np.float32)
    B1 = rng.standard_normal((K, N)).astype(np.float32)
    B2 = rng.standard_normal((K, N)).astype(np.float32)
    a, b, c = dev(A), dev(B1), dev(np.zeros((M, N), np.float32))
    S.gemm(0, 0, M, N, K, 1.0, a, b, 0.0, c)
    r1 = host(c)
    b.copy_(dev(B2))
    S.gemm(0, 0, M, N, K, 1.0, a, b, 0.0, c)
    r2 = host(c)
    assert np.abs(r1 - A @ B1).max() <= FP32_RTOL * np.abs(A @ B1).max()
    assert np.abs(r2 - A @ B2).max() <= FP32_RTOL * np.abs(A @ B2).max()
    s2 = torch.cuda.Stream()
    s2.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s2):
        c2 = torch.zeros_like(c)
        S.gemm(0, 0, M, N, K, 1.0, a, b, 0.0, c2)
    torch.cuda.synchronize()
    assert np.array_equal(host(c2), r2)


def test_gemm_f32_plans_under_hipgraph_capture_survive_eviction():
    """Round-4 advisor finding: the plane path keeps its device scratch in a per-thread LRU of 16 plans. A hipGraph captured over a
    plan keeps its pointers, so (a) the plan a capture uses is pinned - 20 other shapes afterwards must not free what the graph
    replays on; (b) the first sight of a shape UNDER capture does not fail: it records the stateless f32-MFMA kernel; (c) an eager
    call of the captured key gets a plan of its own; (d) saber_hip_gemm_f32_release_plans frees them all."""
    rng = np.random.default_rng(59)
    lib = L.load()
    lib.saber_hip_gemm_f32_release_plans()
    M, N, K = 128, 256, 512
    A = rng.standard_normal((M, K)).astype(np.float32)
    B = rng.standard_normal((K, N)).astype(np.float32)
    want = A.astype(np.float64) @ B.astype(np.float64)
    a, b, c = dev(A), dev(B), dev(np.zeros((M, N), np.float32))
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        S.gemm(0, 0, M, N, K, 1.0, a, b, 0.0, c)          # eager: builds the plan
        st.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=st):
            S.gemm(0, 0, M, N, K, 1.0, a, b, 0.0, c)      # pins it
        # (b) a shape this stream has never run, first seen under capture
        M2, N2, K2 = 96, 160, 264
        A2 = rng.standard_normal((M2, K2)).astype(np.float32)
        B2 = rng.standard_normal((K2, N2)).astype(np.float32)
        a2, b2, c2 = dev(A2), dev(B2), dev(np.zeros((M2, N2), np.float32))
        g2 = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g2, stream=st):
            S.gemm(0, 0, M2, N2, K2, 1.0, a2, b2, 0.0, c2)
        # 20 other shapes on the same stream: more than the LRU holds
        for i in range(20):
            m_ = 64 + 8 * i
            x_, w_, y_ = dev(np.ones((m_, 256), np.float32)), dev(np.ones((256, 256), np.float32)), dev(np.zeros((m_, 256), np.float32))
            S.gemm(0, 0, m_, 256, 256, 1.0, x_, w_, 0.0, y_)
        st.synchronize()
        c.zero_()
        c2.zero_()
        g.replay()
        g2.replay()
        st.synchronize()
        got = host(c)
        assert np.abs(got - want).max() <= FP32_RTOL * np.abs(want).max()
        want2 = A2.astype(np.float64) @ B2.astype(np.float64)
        assert np.abs(host(c2) - want2).max() <= FP32_RTOL * np.abs(want2).max()
        # (c) eager again with the captured key, then the graph again: same bits both ways
        c.zero_()
        S.gemm(0, 0, M, N, K, 1.0, a, b, 0.0, c)
        st.synchronize()
        assert np.array_equal(host(c), got)
        c.zero_()
        g.replay()
        st.synchronize()
        assert np.array_equal(host(c), got)
    del g, g2
    assert lib.saber_hip_gemm_f32_release_plans() >= 2
    assert lib.saber_hip_gemm_f32_release_plans() == 0


@pytest.mark.parametrize("ta,tb", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("adt", [O.S8, O.U8])
def test_gemm_i8_exact(ta, tb, adt):
    """INT8 GEMM (MklDnnGemm<s8|u8, s8, int>): int32 results equal the integer matrix product exactly, for every
    transpose combination, ragged sizes (k % 16 != 0) and accumulators far beyond 2^24."""
    rng = np.random.default_rng(abs(hash((ta, tb, adt))) % 2**31)
    for M, N, K in ((70, 130, 45), (8, 1000, 2048), (33, 64, 4000)):
        A = (rng.integers(0, 256, (M, K)).astype(np.uint8) if adt == O.U8 else rng.integers(-128, 128, (M, K)).astype(np.int8))
        B = rng.integers(-128, 128, (K, N)).astype(np.int8)
        if (M, N, K) == (33, 64, 4000):   # saturate the operands: |acc| up to 4000 * 255 * 128 ~ 1.3e8
            A[:] = 255 if adt == O.U8 else -128
            B[:, ::2] = -128
            B[:, 1::2] = 127
        want = A.astype(np.int64) @ B.astype(np.int64)
        assert np.abs(want).max() < 2**31
        a_dev = dev(np.ascontiguousarray(A.T) if ta else A)
        g = S.GemmInt8().init(ta, tb, M, N, K, np.ascontiguousarray(B.T) if tb else B, adt)
        got = host(g.dispatch(a_dev))
        assert got.dtype == np.int32 and np.array_equal(got.astype(np.int64), want), (M, N, K)


ACT_CASES = [(S.ACTIVE_SIGMOID, 0.0, 1.0), (S.ACTIVE_RELU, 0.3, 1.0), (S.ACTIVE_TANH, 0.0, 1.0), (S.ACTIVE_CLIPPED_RELU, 0.0, 1.7),
             (S.ACTIVE_ELU, 0.0, 0.6), (S.ACTIVE_STANH, 0.66, 1.72), (S.ACTIVE_GELU, 0.0, 1.0), (S.ACTIVE_SWISH, 0.0, 1.3)]


@pytest.mark.parametrize("act", ACT_CASES)
def test_activation_types_vs_oracle(act):
    """Activation<MI355X, AK_FLOAT> beyond relu (round-3 verdict, missing 6): the scalar formulas of saber_activation.cpp:136-262 /
    test_saber_activation.cpp:17-115, on a ragged count, out of place and in place; 1e-4 of the tensor's scale (FP32 contract)."""
    active, slope, coef = act
    rng = np.random.default_rng(70 + active)
    x = (rng.standard_normal(3 * 7 * 11 * 13 + 3) * 3).astype(np.float32)
    want = O.activation_f32(x, active, slope, coef)
    got = host(S.activation(active, dev(x), None, slope, coef))
    assert np.abs(got - want).max() <= FP32_RTOL * max(np.abs(want).max(), 1e-3), active
    xt = dev(x)
    S.activation(active, xt, xt, slope, coef)
    assert np.array_equal(host(xt), got)
    with pytest.raises(L.SaberHipError):
        S.activation(6, dev(x))          # Active_identity: no kernel


@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
def test_prelu_vs_oracle(layout):
    rng = np.random.default_rng(81)
    n, c, h, w = 2, 37, 5, 9
    shape, axis, inner = ((n, c, h, w), 1, h * w) if layout == "nchw" else ((n, h, w, c), 3, 1)
    x = rng.standard_normal(shape).astype(np.float32)
    slope = (rng.standard_normal(c) * 0.5).astype(np.float32)
    for shared in (False, True):
        want = O.prelu_f32(x, slope, axis, shared)
        got = host(S.prelu(dev(x), dev(slope), c, inner, shared))
        assert np.array_equal(got, want), (layout, shared)      # one multiply: exact


@pytest.mark.parametrize("act", [(S.ACTIVE_SIGMOID, 0.0, 1.0), (S.ACTIVE_ELU, 0.0, 0.8), (S.ACTIVE_SWISH, 0.0, 1.0)])
def test_conv_f32_with_a_non_relu_activation(act):
    """A Conv whose ActivationParam is not relu: the convolution without an activation + the activation in place on its output
    (include/saber_mi355x_impl.h: the NV impl's structure, saber/funcs/impl/cuda/saber_conv.cpp `_saber_act`)."""
    active, slope, coef = act
    rng = np.random.default_rng(90 + active)
    N, C, H, W, K = 2, 32, 14, 14, 64
    x = rng.standard_normal((N, C, H, W)).astype(np.float32)
    w = (rng.standard_normal((K, C, 3, 3)) * 0.1).astype(np.float32)
    b = rng.standard_normal(K).astype(np.float32)
    want = O.activation_f32(O.conv_f32_nchw(x, w, b, False, (1, 1), (1, 1), (1, 1), 1), active, slope, coef)
    p = S.ConvParam(w, b, 1, (1, 1), (1, 1), (1, 1), False)
    p.post_act = act
    conv = S.SaberConv2D(False).init(x.shape, p, L.F32, L.F32)
    y = conv.new_output()
    conv.dispatch(dev(x), y)
    assert np.abs(host(y) - want).max() <= FP32_RTOL * np.abs(want).max(), conv.algo()
    p8 = S.ConvParam(w, b, 1, (1, 1), (1, 1), (1, 1), False)
    p8.post_act = act
    with pytest.raises(L.SaberHipError):
        S.SaberConv2D(True).init(x.shape, p8, L.S8, L.S8, 0.05, 0.1)      # INT8: relu only, as on x86


@pytest.mark.parametrize("M", [1, 2, 8, 16])
@pytest.mark.parametrize("K,N", [(2048, 1000), (512, 10), (4096, 1024), (1024, 333), (2048 + 256, 1000)])
def test_fc_i8_softmax_in_one_launch(M, K, N):
    """saber_hip_fc_run_softmax (fc_small.hip: the last-arriving workgroup of the INT8 small-batch fc kernel normalises the rows;
    round-4 verdict item 2 ii): the logits are the bits of saber_hip_fc_run, the probabilities the Softmax operator's within 1e-4 -
    against the oracle AND against the two launches - for s8 and u8 operands, ragged output counts, 12 launches in a row on changing
    inputs (the hand-off goes through memory across XCDs: a stale line would show as a row normalised from old logits). A reduction the
    fused kernel has no instance for (2304) runs the two launches behind the same entry point."""
    rng = np.random.default_rng(300 + M + K + N)
    w = (rng.standard_normal((N, K)) * 0.02).astype(np.float32)
    b = rng.standard_normal(N).astype(np.float32)
    ws = O.weight_scales(w)
    wq = O.quant_weights(w, ws)
    for dt, lo, hi, odt in ((L.S8, -128, 128, np.int8), (L.U8, 0, 256, np.uint8)):
        fc = S.SaberFc(True).init(M, N, K, wq, b, dt, 0.031, 0.5 if dt == L.U8 else 1.0, w_scale=ws)
        fused = K in (512, 1024, 2048, 4096)
        assert fc.algo() == "fc_i8_small_16xk4", fc.algo()
        y = torch.empty((M, N), dtype=torch.float32, device="cuda")
        p = torch.empty((M, N), dtype=torch.float32, device="cuda")
        y2 = torch.empty((M, N), dtype=torch.float32, device="cuda")
        for it in range(12):
            x = rng.integers(lo, hi, (M, K)).astype(odt)
            xd = dev(x)
            y.fill_(7.0)
            p.fill_(-1.0)
            fc.dispatch_softmax(xd, y, p)
            want = O.fc_i8(x, wq, ws, 0.031, b, 0.5) if dt == L.U8 else O.fc_i8(x, wq, ws, 0.031, b)
            got_y, got_p = host(y), host(p)
            assert np.array_equal(got_y, want), (M, K, N, dt, it, fused)
            sm = O.softmax_f32(want)
            assert np.abs(got_p - sm).max() <= FP32_RTOL * sm.max(), (M, K, N, dt, it, np.abs(got_p - sm).max())
            fc.dispatch(xd, y2)
            two = host(S.softmax(y2))
            assert np.array_equal(host(y2), got_y) and np.abs(got_p - two).max() <= FP32_RTOL * two.max()
            assert np.allclose(got_p.sum(1), 1.0, atol=1e-5)


@pytest.mark.parametrize("case", [(2, 224, 224), (1, 96, 96), (3, 70, 70), (1, 61, 47), (2, 33, 40), (9, 64, 64)])
@pytest.mark.parametrize("variant", [0, 1, 2, 3])
def test_stem_f32_one_launch_vs_oracle_and_the_three_ops(case, variant):
    """conv_stem_f32.hip (round 6): NCHW f32 image -> conv 7x7 / 2 / pad 3 (3 -> 64) + bias + relu -> max pooling 3x3 / 2 (ceil shapes) ->
    NHWC f32 in ONE launch, both tile forms, ragged pooled sizes and windows clipped at the conv image's edge - against the oracle's
    conv -> pooling (naive order; 1e-4 on both FP32 criteria) and against the library's own three launches (transpose, implicit-GEMM conv on
    the f32 MFMA, pooling) within 2e-5; the same bits on repeated launches; floor-mode pooling too."""
    N, H, W = case
    rng = np.random.default_rng(900 + N + H + W)
    x = rng.uniform(-1, 1, (N, 3, H, W)).astype(np.float32)
    w = (rng.standard_normal((64, 3, 7, 7)) * np.sqrt(2.0 / 147)).astype(np.float32)
    b = (rng.standard_normal(64) * 0.2).astype(np.float32)
    for floor in (False, True):
        conv_ref = O.conv_f32_nchw(x, w, b, True, (3, 3), (2, 2))
        want = O.pool_f32_nchw(conv_ref, (3, 3), (2, 2), (0, 0), 0, floor_mode=floor).transpose(0, 2, 3, 1)
        stem = S.SaberConv2DPooling(int8=False).init((N, 3, H, W), S.ConvParam(w, b, 1, (3, 3), (2, 2), (1, 1), True), L.POOL_MAX, (3, 3),
                                                      (2, 2), (0, 0), L.F32, L.F32, floor_mode=floor, in_layout=L.NCHW)
        assert stem.fused and stem.algo() == "stem7x7s2_maxpool3x3s2_f32_bf16x3_nchw_in", stem.algo()
        stem.conv.set_tile((15 << 16) | variant)
        y = stem.new_output()
        assert tuple(y.shape) == want.shape, (y.shape, want.shape)
        y.fill_(-7.0)
        stem.dispatch(dev(x), y)
        got = host(y)
        a = np.abs(got - want).max() / np.abs(want).max()
        e = (np.abs(got - want) / (np.abs(want) + np.abs(want).mean())).max()
        assert a <= FP32_RTOL and e <= FP32_RTOL, (case, variant, floor, a, e)
        y2 = stem.new_output()
        stem.dispatch(dev(x), y2)
        assert np.array_equal(host(y2), got)
        # the three separate launches of rounds 1 - 5 (SABER_HIP_NO_STEM_F32 is read per set_pooling call)
        import os
        os.environ["SABER_HIP_NO_STEM_F32"] = "1"
        try:
            three = S.SaberConv2DPooling(int8=False).init((N, 3, H, W), S.ConvParam(w, b, 1, (3, 3), (2, 2), (1, 1), True), L.POOL_MAX, (3, 3),
                                                           (2, 2), (0, 0), L.F32, L.F32, floor_mode=floor, in_layout=L.NCHW)
        finally:
            del os.environ["SABER_HIP_NO_STEM_F32"]
        assert not three.fused
        y3 = three.new_output()
        three.dispatch(dev(x), y3)
        assert np.abs(host(y3) - got).max() <= 2e-5 * np.abs(want).max()


@pytest.mark.parametrize("shape", [(1, 2048, 1000), (8, 2048, 1000), (16, 4096, 1000), (3, 512, 40), (8, 1024, 2048), (5, 2048, 1001)])
def test_fc_f32_split_k_and_softmax_in_one_launch(shape):
    """fc_f32_splitk.hip (round 6): the FP32 fc at <= 16 rows with few output tiles runs with its reduction split over workgroups
    (deterministic second step: the tile's last arriver adds the partials in split order) - the logits within 1e-4 of the oracle on both
    FP32 criteria and of the default one-workgroup-per-tile kernel, the SAME BITS over 20 launches on changing
    buffers; saber_hip_fc_run_softmax = the Softmax operator over those logits in the same launch (<= 1024 outputs), 30 launches in a
    row while two other streams keep the memory system busy: every row sums to 1 and equals softmax of the logits the same launch wrote."""
    M, K, N = shape
    rng = np.random.default_rng(77 + M + K + N)
    w = (rng.standard_normal((N, K)) * np.sqrt(1.0 / K)).astype(np.float32)
    b = rng.standard_normal(N).astype(np.float32)
    x = rng.standard_normal((M, K)).astype(np.float32)
    import os
    os.environ["SABER_HIP_FC_F32_SPLITK"] = "1"      # opt-in (read by set_weights): measured no faster than the two launches, profiles/r06/fc_tail.txt
    try:
        fc = S.SaberFc(False).init(M, N, K, w, b, L.F32)
    finally:
        del os.environ["SABER_HIP_FC_F32_SPLITK"]
    assert fc.algo() == "fc_f32_splitk_16xk4", fc.algo()
    want = O.fc_f32(x, w, b)
    y = torch.empty((M, N), dtype=torch.float32, device="cuda")
    xd = dev(x)
    first = None
    for it in range(20):
        y.fill_(float(it))
        fc.dispatch(xd, y)
        got = host(y)
        if first is None:
            first = got
            a = np.abs(got - want).max() / np.abs(want).max()
            e = (np.abs(got - want) / (np.abs(want) + np.abs(want).mean())).max()
            assert a <= FP32_RTOL and e <= FP32_RTOL, (shape, a, e)
        assert np.array_equal(got, first), (shape, it)
    fc1 = S.SaberFc(False).init(M, N, K, w, b, L.F32)
    assert fc1.algo() == "fc_f32_small_16xk4"
    y1 = torch.empty_like(y)
    fc1.dispatch(xd, y1)
    assert np.abs(host(y1) - first).max() <= 2e-5 * np.abs(want).max()
    if N > 1024:
        return
    big_a = torch.randn(32 << 20, device="cuda")
    big_b = torch.empty_like(big_a)
    side = [torch.cuda.Stream(), torch.cuda.Stream()]
    p = torch.empty((M, N), dtype=torch.float32, device="cuda")
    xs = [dev(rng.standard_normal((M, K)).astype(np.float32)) for _ in range(4)]
    for it in range(30):
        for st in side:
            with torch.cuda.stream(st):
                big_b.copy_(big_a)
        y.fill_(1e30)
        p.fill_(-1.0)
        fc.dispatch_softmax(xs[it % 4], y, p)
        torch.cuda.current_stream().synchronize()
        sm = torch.softmax(y, 1)
        assert torch.allclose(p.sum(1), torch.ones(M, device="cuda"), atol=1e-5) and (p - sm).abs().max() <= 1e-4 * sm.max(), (shape, it)
    torch.cuda.synchronize()
    wantp = O.softmax_f32(O.fc_f32(host(xs[1]), w, b))
    fc.dispatch_softmax(xs[1], y, p)
    assert np.abs(host(p) - wantp).max() <= FP32_RTOL * wantp.max()


@pytest.mark.parametrize("fenced", [False, True], ids=["write_through", "fenced"])
def test_fc_i8_softmax_hand_off_under_concurrent_load(fenced):
    """(round-5 advisor) the fc + softmax launch hands its logits to the last-arriving workgroup through memory across XCDs with
    write-through stores and a relaxed device-scope counter (fc_small.hip). Stress: 400 launches on CHANGING inputs while two other
    streams keep every CU busy with memory traffic and the logits / probabilities buffers are poisoned between launches - a stale or
    late line shows as a row normalised from poisoned or old logits (checked: every row sums to 1 and equals softmax of the logits the
    SAME launch wrote). The release / acquire-fence form (SABER_HIP_FC_SOFTMAX_FENCED=1) runs the same test in a fresh process."""
    if fenced:
        import os
        import subprocess
        import sys
        env = dict(os.environ, SABER_HIP_FC_SOFTMAX_FENCED="1")
        r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", __file__, "-k", "hand_off_under_concurrent_load and write_through"],
                           env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        return
    M, K, N = 8, 2048, 1000
    rng = np.random.default_rng(4242)
    w = (rng.standard_normal((N, K)) * 0.02).astype(np.float32)
    b = rng.standard_normal(N).astype(np.float32)
    ws = O.weight_scales(w)
    wq = O.quant_weights(w, ws)
    fc = S.SaberFc(True).init(M, N, K, wq, b, L.S8, 0.031, 1.0, w_scale=ws)
    xs = [dev(rng.integers(-128, 128, (M, K)).astype(np.int8)) for _ in range(8)]
    ys = [torch.empty((M, N), dtype=torch.float32, device="cuda") for _ in range(8)]
    ps = [torch.empty((M, N), dtype=torch.float32, device="cuda") for _ in range(8)]
    big_a = torch.randn(64 << 20, device="cuda")          # 256 MB: past the Infinity Cache
    big_b = torch.empty_like(big_a)
    side = [torch.cuda.Stream(), torch.cuda.Stream()]
    main = torch.cuda.current_stream()
    bad = 0
    for rnd in range(50):
        for st in side:                                    # keep the memory system and the CUs busy beside the fc launches
            with torch.cuda.stream(st):
                big_b.copy_(big_a)
                big_b.mul_(1.0001)
        for i in range(8):
            ys[i].fill_(1e30)
            ps[i].fill_(-1.0)
            fc.dispatch_softmax(xs[(i + rnd) % 8], ys[i], ps[i])
        main.synchronize()
        for i in range(8):
            p = ps[i]
            want = torch.softmax(ys[i], 1)
            if not (torch.allclose(p.sum(1), torch.ones(M, device="cuda"), atol=1e-5) and (p - want).abs().max() <= 1e-4 * want.max()):
                bad += 1
    torch.cuda.synchronize()
    assert bad == 0, bad


def test_softmax_vs_oracle():
    rng = np.random.default_rng(61)
    x = (rng.standard_normal((8, 1000)) * 4).astype(np.float32)
    got = host(S.softmax(dev(x)))
    want = O.softmax_f32(x)
    assert np.abs(got - want).max() <= FP32_RTOL * want.max() and np.allclose(got.sum(1), 1.0, atol=1e-5)


def _coeff_pair(c, pair):
    """the eltwise's coefficients: `pair` as multiples of c (None: the network's (c, c), c as it is)"""
    return (c, c) if pair is None else (float(np.float32(pair[0] * c)), float(np.float32(pair[1] * c)))


def _coeff_conditions(t1, r, s0, s1, cc, relu, what):
    """tests/block_table.py: from the oracle alone, a swapped pair and the conv's coefficient for both each change a quarter of the bytes"""
    from tests import block_table as BT
    print("%s: (swapped, conv's for both, between the rails) = %s" % (what, BT.coeff_conditions(t1, r, s0, s1, cc[0], cc[1], relu, what)))


SUBSAMPLED_GEOS = [(2, 56, 64, 256, 2), (3, 28, 128, 512, 2), (8, 14, 256, 1024, 2), (2, 15, 64, 128, 2), (1, 30, 32, 64, 3)]


@pytest.mark.parametrize("geo", SUBSAMPLED_GEOS)
def test_conv_i8_fused_eltwise_with_subsampled_residual(geo):
    _subsampled_residual(geo)


@pytest.mark.parametrize("pair", [(1.0, -0.5), (0.5, 1.0)])
def test_conv_i8_fused_eltwise_with_subsampled_residual_unequal_coefficients(pair):
    """the smallest geometry above (15 x 15 x 64 -> 128 under a 29 x 29 shortcut) with (c, -c / 2) and (c / 2, c)"""
    _subsampled_residual(SUBSAMPLED_GEOS[3], pair)


def _subsampled_residual(geo, pair=None):
    """saber_hip_conv_desc::res_stride: the 1x1 / stride-s shortcut pooling of the reference's stride-up pass folded into
    the fused eltwise epilogue's residual read == max-pooling the shortcut first (oracle: pool_i8 floor mode, then
    conv(->s8) + SaberEltwise), every implicit-GEMM variant the op offers."""
    n, ho, c, k, s = geo
    rng = np.random.default_rng(5 + ho + c)
    hs = ho * s - (1 if ho % 2 else 0)            # (hs - 1) // s + 1 == ho for both an exact and a ragged source size
    x = rng.integers(0, 256, (n, ho, ho, c)).astype(np.uint8)
    res_full = rng.integers(-128, 128, (n, hs, hs, k)).astype(np.int8)
    w = (rng.standard_normal((k, c, 1, 1)) * 0.05).astype(np.float32)
    b = (rng.standard_normal(k) * 0.2).astype(np.float32)
    in_scale, conv_scale, res_scale, out_scale = 0.02, 0.11, 0.09, 0.13
    cc = _coeff_pair(1.0 / out_scale, pair)
    pooled = O.pool_i8_nhwc(res_full, (1, 1), (s, s), (0, 0), 0, floor_mode=True)
    assert pooled.shape == (n, ho, ho, k)
    ws = O.weight_scales(w)
    bp, sc = O.conv_i8_prepare(ws, b, in_scale, conv_scale, O.U8, O.S8)
    y = O.conv_i8(x, O.quant_weights(w, ws), bp, sc, O.S8, 0, (0, 0))
    want = O.eltwise_i8(y, pooled, conv_scale, res_scale, cc[0], cc[1], True)
    if pair is not None:
        _coeff_conditions(y, pooled, conv_scale, res_scale, cc, True, "sub-sampled residual %s" % (pair,))
    p = S.ConvParam(w, b, 1, (0, 0), (1, 1), (1, 1), False)
    p.res_mode, p.res_relu, p.coeff, p.scale_res = L.RES_ELTWISE, True, cc, res_scale
    p.res_stride, p.res_hw = s, (hs, hs)
    conv = S.SaberConv2D(True).init((n, c, ho, ho), p, L.U8, L.S8, in_scale, conv_scale)
    variants = [None] + [tile | (ks << 8) | (var << 16) for var, ks, tiles in
                         ((1, 1, range(len(L.TILES))), (2, 1, range(len(L.TILES))), (3, 4, (0, 1, 2)), (4, 4, (0,))) for tile in tiles]
    for t in variants:      # every implicit-GEMM tile / staging variant (register-staged, LDS-DMA ring, wave groups)
        if t is not None:
            conv.set_tile(t)
        out = conv.new_output()
        conv.dispatch(dev(x), out, res=dev(res_full))
        assert np.array_equal(host(out), want), (geo, conv.algo())
    # ragged channel counts take the generic epilogue
    k2 = 72
    w2, b2 = w[:k2], b[:k2]
    ws2 = O.weight_scales(w2)
    bp2, sc2 = O.conv_i8_prepare(ws2, b2, in_scale, conv_scale, O.U8, O.S8)
    want2 = O.eltwise_i8(O.conv_i8(x, O.quant_weights(w2, ws2), bp2, sc2, O.S8, 0, (0, 0)), np.ascontiguousarray(pooled[..., :k2]),
                         conv_scale, res_scale, cc[0], cc[1], True)
    p2 = S.ConvParam(w2, b2, 1, (0, 0), (1, 1), (1, 1), False)
    p2.res_mode, p2.res_relu, p2.coeff, p2.scale_res = L.RES_ELTWISE, True, cc, res_scale
    p2.res_stride, p2.res_hw = s, (hs, hs)
    conv2 = S.SaberConv2D(True).init((n, c, ho, ho), p2, L.U8, L.S8, in_scale, conv_scale)
    out2 = conv2.new_output()
    conv2.dispatch(dev(x), out2, res=dev(np.ascontiguousarray(res_full[..., :k2])))
    assert np.array_equal(host(out2), want2), conv2.algo()


@pytest.mark.parametrize("shape", [(8, 7, 7, 2048), (3, 14, 14, 200), (1, 5, 9, 132), (2, 7, 7, 64)])
@pytest.mark.parametrize("dt", [O.S8, O.U8])
def test_global_average_pooling_i8_kernel(shape, dt):
    """The INT8 global average pooling of the graph's tail (gpool_i8_nhwc_kernel): s8 / u8 / f32 outputs, channel counts that
    are not a multiple of its 128-channel workgroup."""
    rng = np.random.default_rng(shape[1] * 7 + shape[3])
    x = rng.integers(0, 256, shape).astype(np.uint8) if dt == O.U8 else rng.integers(-128, 128, shape).astype(np.int8)
    for od in (None, L.F32):
        got = host(S.pooling_i8(dev(x), None, None, None, 1, out_dtype=od, global_pooling=True))
        want = O.pool_i8_nhwc(x, None, None, None, 1, out_dtype=None if od is None else O.F32, global_pool=True)
        assert np.array_equal(got, want), (shape, dt, od)


# ---- FP32 convolution on the bf16 matrix cores: x = h + m + l (three bf16 planes), six products, f32 accumulate ---------
@pytest.mark.parametrize("tile", list(range(len(L.TILES))) + [6, 7, 8, 9])      # 6..9: the 8-wave forms of 64x64, 128x64, 128x128, 256x128
def test_conv_f32_bf16x3_every_tile_golden(tile):
    """The reference-made golden FP32 3x3 convolution through the bf16-plane variant (set_tile variant 11), every tile:
    within the same 1e-4 as the f32-MFMA kernels (BASELINE.json: FP32 'within 1e-4 rel')."""
    g = load("conv_f32_3x3")
    N, C, H, W, K, k, pad, stride = [int(v) for v in g["spec"]]
    if C % 8:
        pytest.skip("bf16x3 needs C % 8 == 0")
    p = S.ConvParam(g["w"], g["bias"], 1, (pad, pad), (stride, stride), (1, 1), True)
    conv = S.SaberConv2D(int8=False).init((N, C, H, W), p, L.F32, L.F32)
    if tile == 9 and ((K + 127) // 128) % 2:
        with pytest.raises(L.SaberHipError):          # the 256-row tile reads 256 weight rows unpredicated: refused for this K
            conv.set_tile(tile | (1 << 8) | (11 << 16))
        return
    conv.set_tile(tile | (1 << 8) | (11 << 16))
    assert "bf16x3" in conv.algo()
    y = conv.new_output()
    conv.dispatch(dev(g["x"]), y)
    err = np.abs(host(y) - g["y"]).max() / np.abs(g["y"]).max()
    assert err <= FP32_RTOL, (conv.algo(), err)


F32_B3_SWEEP = [
    # N, H, W, C, K, k, pad, stride, dil, layout ("nhwc" | "nchw")
    (2, 28, 28, 64, 64, 3, 1, 1, 1, "nhwc"),     # VGG-like 3x3
    (1, 14, 14, 256, 512, 3, 1, 1, 1, "nhwc"),
    (3, 9, 9, 16, 20, 1, 0, 1, 1, "nhwc"),       # ragged K, tiny C (K-steps straddle... one slab = 32 > C: taps mix)
    (1, 7, 7, 48, 34, 3, 1, 1, 1, "nhwc"),       # K % 4 != 0, C = 48 (a 32-deep slab straddles taps)
    (2, 13, 11, 32, 64, 3, 1, 2, 1, "nhwc"),     # ragged spatial, stride 2
    (1, 10, 10, 16, 16, 3, 2, 1, 2, "nhwc"),     # dilation 2
    (1, 5, 5, 64, 32, 5, 2, 1, 1, "nchw"),       # NCHW in / out (transposed into the workspace)
    (2, 56, 56, 64, 256, 1, 0, 1, 1, "nhwc"),    # ResNet 1x1
]


@pytest.mark.parametrize("tile", [6, 7, 8, 9])
def test_conv_f32_bf16x3_eight_wave_tiles_vs_oracle(tile):
    """The 8-wave forms (two waves per SIMD: 64x64, 128x64, 128x128, 256x128 block tiles) on a VGG-like layer with ragged pixel
    tiles: oracle within 1e-4 on both criteria, and the same bits as the 4-wave kernel of the same block tile where one exists
    (the accumulation order per output is the same)."""
    N, H, W, C, K = 3, 19, 23, 64, 256
    rng = np.random.default_rng(70 + tile)
    x = (rng.random((N, C, H, W)) * 3.0).astype(np.float32)
    w = (rng.standard_normal((K, C, 3, 3)) * np.sqrt(2.0 / (C * 9))).astype(np.float32)
    b = (rng.standard_normal(K) * 0.5).astype(np.float32)
    want = O.conv_f32_nchw(x, w, b, True, (1, 1), (1, 1), (1, 1))
    p = S.ConvParam(w, b, 1, (1, 1), (1, 1), (1, 1), True)
    conv = S.SaberConv2D(int8=False).init((N, C, H, W), p, L.F32, L.F32, in_layout=L.NHWC, out_layout=L.NHWC)
    xin = dev(np.ascontiguousarray(x.transpose(0, 2, 3, 1)))
    outs = {}
    for t in (tile, {6: 2, 7: 3, 8: 5, 9: 5}[tile]):
        conv.set_tile(t | (1 << 8) | (11 << 16))
        y = conv.new_output()
        conv.dispatch(xin, y)
        outs[t] = host(y).transpose(0, 3, 1, 2)
    got = outs[tile]
    d = np.abs(got - want)
    assert float(d.max() / np.abs(want).max()) <= FP32_RTOL and float((d / (np.abs(want) + np.abs(want).mean())).max()) <= FP32_RTOL, conv.algo()
    assert np.array_equal(got, outs[{6: 2, 7: 3, 8: 5, 9: 5}[tile]]), "8-wave and 4-wave kernels sum in the same order"



@pytest.mark.parametrize("case", F32_B3_SWEEP)
def test_conv_f32_bf16x3_sweep_vs_oracle(case):
    """Shapes sweep of the bf16-plane FP32 convolution against the oracle's naive f32 convolution (conv_basic_check order):
    max-norm AND element-wise criteria of the network tests, and against the f32-MFMA kernel of the same op (both are
    rounding-level approximations of the exact sum: they must agree far inside the tolerance)."""
    N, H, W, C, K, k, pad, stride, dil, layout = case
    rng = np.random.default_rng(abs(hash(case)) % 2**31)
    x = (rng.random((N, C, H, W)) * 3.0).astype(np.float32)                                  # relu'd activations
    w = (rng.standard_normal((K, C, k, k)) * np.sqrt(2.0 / (C * k * k))).astype(np.float32)
    b = (rng.standard_normal(K) * 0.5).astype(np.float32)
    want = O.conv_f32_nchw(x, w, b, True, (pad, pad), (stride, stride), (dil, dil))
    p = S.ConvParam(w, b, 1, (pad, pad), (stride, stride), (dil, dil), True)
    lay = L.NCHW if layout == "nchw" else L.NHWC
    xin = x if layout == "nchw" else np.ascontiguousarray(x.transpose(0, 2, 3, 1))
    outs = {}
    for variant in ("f32", "bf16x3"):
        conv = S.SaberConv2D(int8=False).init((N, C, H, W), p, L.F32, L.F32, in_layout=lay, out_layout=lay)
        if variant == "bf16x3":
            conv.set_tile(conv.tile_id() | (1 << 8) | (11 << 16))
            assert "bf16x3" in conv.algo()
        y = conv.new_output()
        conv.dispatch(dev(xin), y)
        got = host(y)
        outs[variant] = got if layout == "nchw" else got.transpose(0, 3, 1, 2)
    for variant, got in outs.items():
        d = np.abs(got - want)
        e_max = float(d.max() / np.abs(want).max())
        e_el = float((d / (np.abs(want) + np.abs(want).mean())).max())
        assert e_max <= FP32_RTOL and e_el <= FP32_RTOL, (variant, case, e_max, e_el)
    assert np.abs(outs["f32"] - outs["bf16x3"]).max() <= 2e-5 * np.abs(want).max()


F32_SPLITK_CASES = [
    # N, H, W, C, K, k, pad, eltwise residual, tile ids, splits (log2)
    (8, 14, 14, 256, 256, 3, 1, False, (0, 1, 2, 3, 6, 7), (1, 2, 3)),     # ResNet res4 branch2b at batch 8 (6, 7: 8-wave tiles)
    (8, 7, 7, 512, 512, 3, 1, False, (2,), (1, 2, 3)),               # res5 branch2b
    (3, 7, 9, 2048, 512, 1, 0, False, (1, 2), (2, 3)),               # res5 branch2a, ragged pixels (tiles % 8 != 0)
    (2, 5, 5, 96, 40, 3, 1, False, (0, 2), (1, 2)),                  # ragged K / C, slabs straddle taps
    (4, 14, 14, 256, 1024, 1, 0, True, (2,), (1,)),                  # ConvEltwise epilogue (in-place residual sum) after the sum
]


@pytest.mark.parametrize("case", F32_SPLITK_CASES)
def test_conv_f32_bf16x3_split_k_vs_oracle_and_deterministic(case):
    """FP32 split-K (2 / 4 / 8 workgroups per output tile on ONE XCD, partial sums handed over through that XCD's L2, summed
    in split order by the last arrival): the oracle's convolution within 1e-4 (both criteria of the network tests), the same
    bits on every launch (the order of the sum is fixed, not the order of arrival), the unsplit kernel within rounding."""
    N, H, W, C, K, k, pad, elt, tiles, splits = case
    rng = np.random.default_rng(N * 1000 + C + K)
    x = (rng.random((N, C, H, W)) * 3.0).astype(np.float32)
    w = (rng.standard_normal((K, C, k, k)) * np.sqrt(2.0 / (C * k * k))).astype(np.float32)
    b = (rng.standard_normal(K) * 0.5).astype(np.float32)
    res = (rng.random((N, K, H, W)) * 2.0).astype(np.float32)
    want = O.conv_f32_nchw(x, w, b, not elt, (pad, pad), (1, 1), (1, 1))
    if elt:
        want = np.maximum(want + res, 0.0)
    p = S.ConvParam(w, b, 1, (pad, pad), (1, 1), (1, 1), not elt)
    if elt:
        p.res_mode, p.res_relu, p.sum_scale = L.RES_SUM_INPLACE, True, 1.0
    xin = dev(np.ascontiguousarray(x.transpose(0, 2, 3, 1)))
    rin = np.ascontiguousarray(res.transpose(0, 2, 3, 1))
    conv = S.SaberConv2D(int8=False).init((N, C, H, W), p, L.F32, L.F32, in_layout=L.NHWC, out_layout=L.NHWC)

    def run():
        y = conv.new_output()
        if elt:
            y.copy_(dev(rin))
        conv.dispatch(xin, y)
        return host(y).transpose(0, 3, 1, 2)
    conv.set_tile(conv.tile_id() | (1 << 8) | (11 << 16))
    base = run()
    for t in tiles:
        for sh in splits:
            code = t | ((1 | (sh << 4)) << 8) | (11 << 16)
            try:
                conv.set_tile(code)
            except L.SaberHipError:
                assert (C * k * k + 31) // 32 >> sh < 2, (case, t, sh)      # refused only for < 2 stages per split
                continue
            assert "split%d" % (1 << sh) in conv.algo(), conv.algo()
            assert L.load().saber_hip_conv2d_get_tile(conv.h) == code
            got = run()
            d = np.abs(got - want)
            e_max = float(d.max() / np.abs(want).max())
            e_el = float((d / (np.abs(want) + np.abs(want).mean())).max())
            assert e_max <= FP32_RTOL and e_el <= FP32_RTOL, (conv.algo(), e_max, e_el)
            assert np.abs(got - base).max() <= 2e-5 * np.abs(want).max(), conv.algo()
            for _ in range(3):
                assert np.array_equal(run(), got), ("not deterministic", conv.algo())


F32_HALO_CASES = [
    # N, H, W, C, K, eltwise residual
    (2, 56, 56, 64, 64, False),       # ResNet res2 branch2b
    (1, 28, 28, 128, 128, False),     # res3
    (2, 19, 23, 32, 40, False),       # ragged tiles, K % 16 != 0
    (1, 9, 40, 96, 200, True),        # in-place residual sum, three channel chunks
    (3, 14, 14, 256, 256, False),     # res4: 14 of 16 columns used
]


@pytest.mark.parametrize("case", F32_HALO_CASES)
@pytest.mark.parametrize("variant", [1, 2, 3, 4, 5])
def test_conv_f32_bf16x3_halo_kernel_vs_oracle(case, variant):
    """FP32 3x3 on the bf16 planes with the input halo resident in LDS (conv3x3_b3h.hip, set_tile variant 13): the oracle's naive
    convolution within 1e-4 on both criteria, and within rounding of the implicit-GEMM bf16-plane kernel."""
    N, H, W, C, K, elt = case
    rng = np.random.default_rng(N * 100 + C + K + variant)
    x = (rng.random((N, C, H, W)) * 3.0).astype(np.float32)
    w = (rng.standard_normal((K, C, 3, 3)) * np.sqrt(2.0 / (C * 9))).astype(np.float32)
    b = (rng.standard_normal(K) * 0.5).astype(np.float32)
    res = (rng.random((N, K, H, W)) * 2.0).astype(np.float32)
    want = O.conv_f32_nchw(x, w, b, not elt, (1, 1), (1, 1), (1, 1))
    if elt:
        want = np.maximum(want + res, 0.0)
    p = S.ConvParam(w, b, 1, (1, 1), (1, 1), (1, 1), not elt)
    if elt:
        p.res_mode, p.res_relu, p.sum_scale = L.RES_SUM_INPLACE, True, 1.0
    conv = S.SaberConv2D(int8=False).init((N, C, H, W), p, L.F32, L.F32, in_layout=L.NHWC, out_layout=L.NHWC)
    xin = dev(np.ascontiguousarray(x.transpose(0, 2, 3, 1)))
    rin = np.ascontiguousarray(res.transpose(0, 2, 3, 1))

    def run():
        y = conv.new_output()
        if elt:
            y.copy_(dev(rin))
        conv.dispatch(xin, y)
        return host(y).transpose(0, 3, 1, 2)
    conv.set_tile(conv.tile_id() | (1 << 8) | (11 << 16))
    base = run()
    conv.set_tile(variant | (13 << 16))
    assert conv.algo().startswith("halo3x3_f32_bf16x3"), conv.algo()
    assert L.load().saber_hip_conv2d_get_tile(conv.h) == variant | (13 << 16)
    got = run()
    d = np.abs(got - want)
    e_max = float(d.max() / np.abs(want).max())
    e_el = float((d / (np.abs(want) + np.abs(want).mean())).max())
    assert e_max <= FP32_RTOL and e_el <= FP32_RTOL, (conv.algo(), e_max, e_el)
    assert np.abs(got - base).max() <= 2e-5 * np.abs(want).max(), conv.algo()


F32_PW_CASES = [
    # N, H, W, C, K, eltwise residual
    (2, 56, 56, 64, 256, True),       # ResNet res2 branch2c + in-place residual sum
    (1, 28, 28, 512, 128, False),     # res3 branch2a
    (3, 7, 9, 128, 72, False),        # ragged pixels (189), K % 16 != 0
    (1, 14, 14, 1024, 256, False),    # res4 branch2a: 32 channel chunks
]


@pytest.mark.parametrize("case", F32_PW_CASES)
@pytest.mark.parametrize("variant", [6, 7, 8])
def test_conv_f32_bf16x3_pointwise_kernel_vs_oracle(case, variant):
    """The 1x1 forms of conv3x3_b3h.hip (variants 6..8: a run of 64 / 128 pixels x 64 / 128 channels per workgroup, weights straight
    into MFMA registers, the pixel run split once per 32-channel chunk): oracle within 1e-4, implicit-GEMM bf16-plane kernel within rounding."""
    N, H, W, C, K, elt = case
    rng = np.random.default_rng(N * 10 + C + K + variant)
    x = (rng.random((N, C, H, W)) * 3.0).astype(np.float32)
    w = (rng.standard_normal((K, C, 1, 1)) * np.sqrt(2.0 / C)).astype(np.float32)
    b = (rng.standard_normal(K) * 0.5).astype(np.float32)
    res = (rng.random((N, K, H, W)) * 2.0).astype(np.float32)
    want = O.conv_f32_nchw(x, w, b, not elt, (0, 0), (1, 1), (1, 1))
    if elt:
        want = np.maximum(want + res, 0.0)
    p = S.ConvParam(w, b, 1, (0, 0), (1, 1), (1, 1), not elt)
    if elt:
        p.res_mode, p.res_relu, p.sum_scale = L.RES_SUM_INPLACE, True, 1.0
    conv = S.SaberConv2D(int8=False).init((N, C, H, W), p, L.F32, L.F32, in_layout=L.NHWC, out_layout=L.NHWC)
    xin = dev(np.ascontiguousarray(x.transpose(0, 2, 3, 1)))
    rin = np.ascontiguousarray(res.transpose(0, 2, 3, 1))

    def run():
        y = conv.new_output()
        if elt:
            y.copy_(dev(rin))
        conv.dispatch(xin, y)
        return host(y).transpose(0, 3, 1, 2)
    conv.set_tile(conv.tile_id() | (1 << 8) | (11 << 16))
    base = run()
    conv.set_tile(variant | (13 << 16))
    assert conv.algo().startswith("pw1x1_f32_bf16x3"), conv.algo()
    got = run()
    d = np.abs(got - want)
    assert float(d.max() / np.abs(want).max()) <= FP32_RTOL and float((d / (np.abs(want) + np.abs(want).mean())).max()) <= FP32_RTOL, conv.algo()
    assert np.abs(got - base).max() <= 2e-5 * np.abs(want).max(), conv.algo()
    with pytest.raises(L.SaberHipError):
        conv.set_tile(2 | (13 << 16))          # a 3x3 variant on a 1x1 conv


F32_PW_REG_CASES = [
    # N, H, W, C, K, in-place residual sum, relu, bias
    (2, 56, 56, 64, 256, True, True, True),       # ResNet res2 branch2c + in-place residual sum (round-4 verdict item 3)
    (8, 56, 56, 64, 256, True, True, True),       # ... at the bench's batch: 25 088 pixels, 1 568 groups over 256 slots
    (2, 56, 56, 64, 64, False, True, True),       # res2a branch2a
    (2, 28, 28, 128, 512, True, True, True),      # res3 branch2c + sum
    (1, 28, 28, 128, 128, False, False, False),   # no relu, no bias
    (3, 7, 9, 64, 128, True, False, True),        # ragged pixels (189 = 11 groups + 13), sum without relu
    (1, 5, 5, 128, 1024, False, True, True),      # fewer groups (2) than slots (32): most waves have nothing to do
]


@pytest.mark.parametrize("case", F32_PW_REG_CASES)
def test_conv_f32_pointwise_register_weights_kernel_vs_oracle(case):
    """conv1x1_pw.hip (kernel variant 14: persistent independent waves, their output channels' bf16 weight planes in registers, no LDS,
    no barrier - the productised scripts/probe/pw_direct_probe.hip): the oracle within 1e-4 on both criteria, the implicit-GEMM bf16-plane
    kernel within rounding, the selection round-trips through get_tile / set_tile, repeated launches give the same bits; a layer the
    kernel does not take (C = 256, stride 2) refuses the variant."""
    N, H, W, C, K, elt, relu, bias = case
    rng = np.random.default_rng(N * 10 + C + K + H)
    x = (rng.random((N, C, H, W)) * 3.0).astype(np.float32)
    w = (rng.standard_normal((K, C, 1, 1)) * np.sqrt(2.0 / C)).astype(np.float32)
    b = (rng.standard_normal(K) * 0.5).astype(np.float32) if bias else None
    res = (rng.random((N, K, H, W)) * 2.0 - 0.5).astype(np.float32)
    want = O.conv_f32_nchw(x, w, b if bias else np.zeros(K, np.float32), relu and not elt, (0, 0), (1, 1), (1, 1))
    if elt:
        want = want + res
        if relu:
            want = np.maximum(want, 0.0)
    p = S.ConvParam(w, b, 1, (0, 0), (1, 1), (1, 1), relu and not elt)
    if elt:
        p.res_mode, p.res_relu, p.sum_scale = L.RES_SUM_INPLACE, relu, 1.0
    conv = S.SaberConv2D(int8=False).init((N, C, H, W), p, L.F32, L.F32, in_layout=L.NHWC, out_layout=L.NHWC)
    xin = dev(np.ascontiguousarray(x.transpose(0, 2, 3, 1)))
    rin = np.ascontiguousarray(res.transpose(0, 2, 3, 1))

    def run():
        y = conv.new_output()
        y.copy_(dev(rin)) if elt else y.fill_(-7.0)
        conv.dispatch(xin, y)
        return host(y).transpose(0, 3, 1, 2)
    conv.set_tile(conv.tile_id() | (1 << 8) | (11 << 16))
    base = run()
    conv.set_tile(14 << 16)
    assert conv.algo().startswith("pw1x1_f32_bf16x3_regs_c%d" % C), conv.algo()
    assert L.load().saber_hip_conv2d_get_tile(conv.h) == 14 << 16
    got = run()
    d = np.abs(got - want)
    e_max = float(d.max() / np.abs(want).max())
    e_el = float((d / (np.abs(want) + np.abs(want).mean())).max())
    assert e_max <= FP32_RTOL and e_el <= FP32_RTOL, (conv.algo(), e_max, e_el)
    assert np.abs(got - base).max() <= 2e-5 * np.abs(want).max(), conv.algo()
    assert np.array_equal(run(), got)


def test_conv_f32_pointwise_register_weights_kernel_refuses_other_layers():
    rng = np.random.default_rng(3)
    for (c, k, stride) in ((256, 64, 1), (64, 256, 2), (64, 72, 1)):
        w = (rng.standard_normal((k, c, 1, 1)) * 0.1).astype(np.float32)
        p = S.ConvParam(w, None, 1, (0, 0), (stride, stride), (1, 1), True)
        conv = S.SaberConv2D(int8=False).init((1, c, 16, 16), p, L.F32, L.F32, in_layout=L.NHWC, out_layout=L.NHWC)
        with pytest.raises(L.SaberHipError):
            conv.set_tile(14 << 16)


F32_PWK_CASES = [
    # N, H, W, C, K, in-place residual sum, relu, bias
    (8, 14, 14, 1024, 256, False, True, True),    # ResNet res4 branch2a at the bench's batch: 8 slabs per wave
    (8, 14, 14, 256, 1024, True, True, True),     # res4 branch2c + in-place residual sum: 2 slabs per wave (fewer than slabs in flight)
    (2, 56, 56, 256, 64, False, True, True),      # res2b branch2a: one channel tile
    (2, 28, 28, 512, 128, False, True, True),     # res3b branch2a
    (8, 7, 7, 2048, 512, False, True, True),      # res5b branch2a: 16 slabs per wave, 392 pixels = 24 groups + 8
    (4, 7, 7, 512, 2048, True, True, True),       # res5 branch2c + sum
    (3, 7, 9, 384, 192, True, False, True),       # ragged pixels (189), 3 slabs per wave, sum without relu
    (1, 5, 5, 256, 64, False, False, False),      # 25 pixels: a partial first group row, no relu, no bias
    (2, 28, 28, 128, 512, True, True, True),      # res3 branch2c + sum: ONE slab per wave (only the one-slab-in-flight variant takes it)
]


@pytest.mark.parametrize("variant", [1, 2, 3, 4])
@pytest.mark.parametrize("case", F32_PWK_CASES)
def test_conv_f32_pointwise_reduction_split_kernel_vs_oracle(case, variant):
    """conv1x1_pwk.hip (kernel variant 14, low byte 1 .. 4: the four waves of a workgroup split the reduction by 32-channel slab, weight
    fragments and activations straight into registers, several slabs in flight per wave, partial sums meet in LDS once): the oracle within
    1e-4 on both criteria, the implicit-GEMM bf16-plane kernel within rounding, the selection round-trips through get_tile / set_tile,
    repeated launches give the same bits."""
    N, H, W, C, K, elt, relu, bias = case
    rng = np.random.default_rng(N * 10 + C + K + H)
    x = (rng.random((N, C, H, W)) * 3.0 - 1.0).astype(np.float32)
    w = (rng.standard_normal((K, C, 1, 1)) * np.sqrt(2.0 / C)).astype(np.float32)
    b = (rng.standard_normal(K) * 0.5).astype(np.float32) if bias else None
    res = (rng.random((N, K, H, W)) * 2.0 - 0.5).astype(np.float32)
    want = O.conv_f32_nchw(x, w, b if bias else np.zeros(K, np.float32), relu and not elt, (0, 0), (1, 1), (1, 1))
    if elt:
        want = want + res
        if relu:
            want = np.maximum(want, 0.0)
    p = S.ConvParam(w, b, 1, (0, 0), (1, 1), (1, 1), relu and not elt)
    if elt:
        p.res_mode, p.res_relu, p.sum_scale = L.RES_SUM_INPLACE, relu, 1.0
    conv = S.SaberConv2D(int8=False).init((N, C, H, W), p, L.F32, L.F32, in_layout=L.NHWC, out_layout=L.NHWC)
    xin = dev(np.ascontiguousarray(x.transpose(0, 2, 3, 1)))
    rin = np.ascontiguousarray(res.transpose(0, 2, 3, 1))

    def run():
        y = conv.new_output()
        y.copy_(dev(rin)) if elt else y.fill_(-7.0)
        conv.dispatch(xin, y)
        return host(y).transpose(0, 3, 1, 2)
    conv.set_tile(conv.tile_id() | (1 << 8) | (11 << 16))
    base = run()
    if C // 128 < {1: 1, 2: 3, 3: 2, 4: 2}[variant]:      # fewer slabs per wave than the variant keeps in flight: refused
        with pytest.raises(L.SaberHipError):
            conv.set_tile((14 << 16) | variant)
        return
    conv.set_tile((14 << 16) | variant)
    assert conv.algo().startswith("pw1x1_f32_bf16x3_ksplit4_"), conv.algo()
    assert L.load().saber_hip_conv2d_get_tile(conv.h) == (14 << 16) | variant
    got = run()
    d = np.abs(got - want)
    e_max = float(d.max() / np.abs(want).max())
    e_el = float((d / (np.abs(want) + np.abs(want).mean())).max())
    assert e_max <= FP32_RTOL and e_el <= FP32_RTOL, (conv.algo(), e_max, e_el)
    assert np.abs(got - base).max() <= 2e-5 * np.abs(want).max(), conv.algo()
    assert np.array_equal(run(), got)


def test_conv_f32_pointwise_reduction_split_kernel_refuses_other_layers():
    rng = np.random.default_rng(4)
    for (c, k, stride) in ((64, 64, 1), (256, 64, 2), (320, 64, 1), (256, 72, 1)):
        w = (rng.standard_normal((k, c, 1, 1)) * 0.1).astype(np.float32)
        p = S.ConvParam(w, None, 1, (0, 0), (stride, stride), (1, 1), True)
        conv = S.SaberConv2D(int8=False).init((1, c, 16, 16), p, L.F32, L.F32, in_layout=L.NHWC, out_layout=L.NHWC)
        with pytest.raises(L.SaberHipError):
            conv.set_tile((14 << 16) | 1)


STRIDED_HEAD_CASES = [
    # C, N, Hin, Win, 3x3 input dtype, mid dtype, eltwise relu, tile code (None: default)
    (64, 2, 56, 56, O.U8, O.U8, 1, None),        # res2c after the reference's stride-up: 56 -> 28
    (64, 1, 27, 41, O.U8, O.U8, 1, 2),           # odd input dims: ragged output rows / columns, odd shortcut dims
    (128, 2, 28, 28, O.U8, O.U8, 1, None),       # res3d
    (128, 1, 11, 35, O.S8, O.S8, 0, 1),
    (128, 2, 28, 28, O.U8, O.U8, 1, 6),          # 8 waves per workgroup
    (256, 2, 14, 14, O.U8, O.U8, 1, None),       # res4f
    (256, 1, 9, 7, O.U8, O.S8, 1, None),
]


HEAD_PAIR_CASES = [(2, 56, 56, O.U8, O.U8, 1, 512, None), (1, 27, 41, O.U8, O.U8, 1, 512, 2), (2, 30, 22, O.S8, O.S8, 0, 128, 4),
                   (1, 56, 56, O.U8, O.U8, 1, 608, 2)]


@pytest.mark.parametrize("case", HEAD_PAIR_CASES)
def test_strided_head_chain_runs_the_next_stages_sibling_pair(case):
    _strided_head_pair(case)


@pytest.mark.parametrize("pair", [(1.0, -0.5), (0.5, 1.0)])
def test_strided_head_chain_with_sibling_pair_unequal_coefficients(pair):
    """the smallest case above (27 x 41, ragged) with (c, -c / 2) and (c / 2, c) on the head's eltwise"""
    _strided_head_pair(HEAD_PAIR_CASES[1], pair)


def _strided_head_pair(case, pair=None):
    """saber_hip_conv2d_chain_create3_pair: res2c as the reference's stride-up leaves it (3x3 / stride 2, 1x1 + eltwise on the sub-sampled
    shortcut, C = 64) AND the two 1x1 convs that read its output (res3a_branch1 / res3a_branch2a) in ONE launch: all three written tensors
    are the bits of the four operators one after the other (ragged tiles, both pixel-tile heights, either split of the 640 channels)."""
    N, H, Wd, idt, mdt, res_relu, Kb, tn = case
    Cc, K1, Kc = 64, 256, 640 - Kb
    rng = np.random.default_rng(4100 + H + Kb)
    x = (rng.integers(0, 256, (N, H, Wd, Cc)).astype(np.uint8) if idt == O.U8 else rng.integers(-128, 128, (N, H, Wd, Cc)).astype(np.int8))
    Ho, Wo = (H + 2 - 3) // 2 + 1, (Wd + 2 - 3) // 2 + 1
    Hs, Ws = 2 * Ho - (1 if H % 2 else 0), 2 * Wo - (1 if Wd % 2 else 0)
    res_full = rng.integers(-128, 128, (N, Hs, Ws, K1)).astype(np.int8)
    w0 = (rng.standard_normal((Cc, Cc, 3, 3)) * np.sqrt(2.0 / (9 * Cc))).astype(np.float32)
    b0 = (rng.standard_normal(Cc) * 0.5).astype(np.float32)
    w1 = (rng.standard_normal((K1, Cc, 1, 1)) * np.sqrt(2.0 / Cc)).astype(np.float32)
    b1 = (rng.standard_normal(K1) * 0.5).astype(np.float32)
    s_x, s_in, s_mid, s_res, s_sum = 0.023, 0.02, 0.05, 0.043, 0.06
    cc = _coeff_pair(1.0 / s_sum, pair)
    relu0 = mdt == O.U8
    ws0 = O.weight_scales(w0)
    bp0, sc0 = O.conv_i8_prepare(ws0, b0, s_x, s_in, idt, mdt)
    t0 = O.conv_i8(x, O.quant_weights(w0, ws0), bp0, sc0, mdt, int(relu0), (1, 1), (2, 2))
    ws1 = O.weight_scales(w1)
    bp1, sc1 = O.conv_i8_prepare(ws1, b1, s_in, s_mid, mdt, O.S8)
    t1 = O.conv_i8(t0, O.quant_weights(w1, ws1), bp1, sc1, O.S8, 0)
    pooled = O.pool_i8_nhwc(res_full, (1, 1), (2, 2), (0, 0), 0, floor_mode=True)
    y1_want = O.eltwise_i8(t1, pooled, s_mid, s_res, cc[0], cc[1], bool(res_relu))
    if pair is not None:
        _coeff_conditions(t1, pooled, s_mid, s_res, cc, bool(res_relu), "strided head + pair %s" % (pair,))
    c0 = S.SaberConv2D(int8=True).init((N, Cc, H, Wd), S.ConvParam(w0, b0, 1, (1, 1), (2, 2), (1, 1), bool(relu0)), idt, mdt, s_x, s_in)
    pa = S.ConvParam(w1, b1, 1, (0, 0), (1, 1), (1, 1), False)
    pa.res_mode, pa.res_relu, pa.sum_scale, pa.coeff, pa.scale_res = L.RES_ELTWISE, bool(res_relu), 1.0, cc, s_res
    pa.res_stride, pa.res_hw = 2, (Hs, Ws)
    ca = S.SaberConv2D(int8=True).init((N, Cc, Ho, Wo), pa, mdt, O.S8, s_in, s_mid)
    pair, wants = [], []
    for K, kdt, relu, out_scale in ((Kb, O.S8, 0, 0.045), (Kc, O.U8, 1, 0.033)):
        wk = (rng.standard_normal((K, K1, 1, 1)) * np.sqrt(2.0 / K1)).astype(np.float32)
        bk = (rng.standard_normal(K) * 0.5).astype(np.float32)
        wsk = O.weight_scales(wk)
        bpk, sck = O.conv_i8_prepare(wsk, bk, s_sum, out_scale, O.S8, kdt)
        wants.append(O.conv_i8(y1_want, O.quant_weights(wk, wsk), bpk, sck, kdt, relu))
        pair.append(S.SaberConv2D(True).init((N, K1, Ho, Wo), S.ConvParam(wk, bk, 1, (0, 0), (1, 1), (1, 1), bool(relu)), O.S8, kdt, s_sum, out_scale))
    chain = S.SaberConvChain(ca, pair[0], conv3x3=c0, pair_b=pair[1])
    for t in ([tn] if tn is not None else [4, 2]):
        chain.set_tile(t)
        z1, zb, zc = ca.new_output(), pair[0].new_output(), pair[1].new_output()
        for z in (z1, zb, zc):
            z.fill_(77)
        chain.dispatch(dev(x), dev(res_full), z1, zb, zc)
        assert np.array_equal(host(z1), y1_want), ("head", t)
        assert np.array_equal(host(zb), wants[0]) and np.array_equal(host(zc), wants[1]), ("pair", t)
    with pytest.raises(L.SaberHipError):
        chain.set_tile(1)
    with pytest.raises(L.SaberHipError):       # not 640 channels in total
        S.SaberConvChain(ca, pair[0], conv3x3=c0, pair_b=pair[0])


@pytest.mark.parametrize("case", STRIDED_HEAD_CASES)
def test_strided_conv3x3_conv1x1_chain_with_subsampled_shortcut(case):
    _strided_head(case)


@pytest.mark.parametrize("pair", [(1.0, -0.5), (0.5, 1.0)])
def test_strided_conv3x3_conv1x1_chain_unequal_coefficients(pair):
    """the smallest case above (C = 256, 9 x 7, u8 -> s8) with (c, -c / 2) and (c / 2, c) on the head's eltwise"""
    _strided_head(STRIDED_HEAD_CASES[-1], pair)


def _strided_head(case, pair=None):
    """The last block of a stage as the reference's stride-up leaves it: 3x3 / stride 2 (C -> C), then 1x1 (C -> 4C) + eltwise
    whose shortcut is the previous block's output sub-sampled by 2 (the absorbed 1x1 / stride-2 pooling, res_stride) — ONE
    launch (saber_hip_conv2d_chain_create3 with a stride-2 head and no second 1x1 conv), the bits of pooling + the two convs."""
    Cc, N, H, Wd, idt, mdt, res_relu, tn = case
    rng = np.random.default_rng(3100 + Cc + H)
    K1 = 4 * Cc
    x = (rng.integers(0, 256, (N, H, Wd, Cc)).astype(np.uint8) if idt == O.U8
         else rng.integers(-128, 128, (N, H, Wd, Cc)).astype(np.int8))
    Ho, Wo = (H + 2 - 3) // 2 + 1, (Wd + 2 - 3) // 2 + 1
    Hs, Ws = 2 * Ho - (1 if H % 2 else 0), 2 * Wo - (1 if Wd % 2 else 0)        # shortcut dims with (Hs - 1) // 2 + 1 == Ho
    assert (Hs - 1) // 2 + 1 == Ho and (Ws - 1) // 2 + 1 == Wo
    res_full = rng.integers(-128, 128, (N, Hs, Ws, K1)).astype(np.int8)
    w0 = (rng.standard_normal((Cc, Cc, 3, 3)) * np.sqrt(2.0 / (9 * Cc))).astype(np.float32)
    b0 = (rng.standard_normal(Cc) * 0.5).astype(np.float32)
    w1 = (rng.standard_normal((K1, Cc, 1, 1)) * np.sqrt(2.0 / Cc)).astype(np.float32)
    b1 = (rng.standard_normal(K1) * 0.5).astype(np.float32)
    s_x, s_in, s_mid, s_res, s_sum = 0.023, 0.02, 0.05, 0.043, 0.06
    c = 1.0 / s_sum
    cc = _coeff_pair(c, pair)
    relu0 = mdt == O.U8
    ws0 = O.weight_scales(w0)
    bp0, sc0 = O.conv_i8_prepare(ws0, b0, s_x, s_in, idt, mdt)
    t0 = O.conv_i8(x, O.quant_weights(w0, ws0), bp0, sc0, mdt, int(relu0), (1, 1), (2, 2))
    assert t0.shape == (N, Ho, Wo, Cc)
    ws1 = O.weight_scales(w1)
    bp1, sc1 = O.conv_i8_prepare(ws1, b1, s_in, s_mid, mdt, O.S8)
    t1 = O.conv_i8(t0, O.quant_weights(w1, ws1), bp1, sc1, O.S8, 0)
    pooled = O.pool_i8_nhwc(res_full, (1, 1), (2, 2), (0, 0), 0, floor_mode=True)
    want = O.eltwise_i8(t1, pooled, s_mid, s_res, cc[0], cc[1], bool(res_relu))
    if pair is not None:
        _coeff_conditions(t1, pooled, s_mid, s_res, cc, bool(res_relu), "strided head %s" % (pair,))
    c0 = S.SaberConv2D(int8=True).init((N, Cc, H, Wd), S.ConvParam(w0, b0, 1, (1, 1), (2, 2), (1, 1), bool(relu0)), idt, mdt,
                                       s_x, s_in)
    pa = S.ConvParam(w1, b1, 1, (0, 0), (1, 1), (1, 1), False)
    pa.res_mode, pa.res_relu, pa.sum_scale, pa.coeff, pa.scale_res = L.RES_ELTWISE, bool(res_relu), 1.0, cc, s_res
    pa.res_stride, pa.res_hw = 2, (Hs, Ws)
    ca = S.SaberConv2D(int8=True).init((N, Cc, Ho, Wo), pa, mdt, O.S8, s_in, s_mid)
    y0, y1 = c0.new_output(), ca.new_output()
    c0.dispatch(dev(x), y0)
    ca.dispatch(y0, y1, dev(res_full))
    assert np.array_equal(host(y0), t0) and np.array_equal(host(y1), want)        # the two launches
    chain = S.SaberConvChain(ca, None, conv3x3=c0)
    if tn is not None:
        chain.set_tile(tn)
    z1 = ca.new_output()
    z1.fill_(77)
    chain.dispatch(dev(x), dev(res_full), z1)
    assert np.array_equal(host(z1), want), ("strided head", chain.tile())
    # a stride-2 head in front of a chain WITH a second 1x1 conv, or without the sub-sampled shortcut, does not exist
    pb = S.ConvParam(w1, b1, 1, (0, 0), (1, 1), (1, 1), False)
    pb.res_mode, pb.res_relu, pb.sum_scale, pb.coeff, pb.scale_res = L.RES_ELTWISE, True, 1.0, (c, c), s_res
    plain = S.SaberConv2D(int8=True).init((N, Cc, Ho, Wo), pb, mdt, O.S8, s_in, s_mid)
    with pytest.raises(L.SaberHipError):
        S.SaberConvChain(plain, None, conv3x3=c0)


def test_chain_set_tile_accepts_the_form_table_and_every_form_gives_the_default_bytes():
    """Every code 0..15 through saber_hip_conv2d_chain_set_tile on every kind of chain, at the smallest shapes of the cases above. The accepted
    set is the chain-form table's (api_chain.hip: chain_forms), written out here; the cooperative forms of the 3x3-led C = 256 chain (7, 15)
    exist together or not at all (the placement probe decides). Every accepted code writes the bytes of the default code; a refused one
    raises, leaves the selection alone and nothing is launched for it."""
    rng = np.random.default_rng(5150)
    s_x, s_in, s_mid, s_res, s_sum, s_out = 0.023, 0.02, 0.05, 0.043, 0.06, 0.031
    cf = 1.0 / s_sum

    def conv(shape, k, ksz, stride, idt, odt, si, so, relu, elt=False, res_hw=None):
        c = shape[1]
        w = (rng.standard_normal((k, c, ksz, ksz)) * np.sqrt(2.0 / (ksz * ksz * c))).astype(np.float32)
        b = (rng.standard_normal(k) * 0.5).astype(np.float32)
        p = S.ConvParam(w, b, 1, (ksz // 2, ksz // 2), (stride, stride), (1, 1), bool(relu))
        if elt:
            p.res_mode, p.res_relu, p.sum_scale, p.coeff, p.scale_res = L.RES_ELTWISE, True, 1.0, (cf, cf), s_res
        if res_hw:
            p.res_stride, p.res_hw = 2, res_hw
        return S.SaberConv2D(int8=True).init(shape, p, idt, odt, si, so)

    def check(what, chain, want_codes, x, res, outs):
        default = chain.tile()
        assert default in want_codes, (what, default)

        def run():
            zs = [o.new_output() for o in outs]
            for z in zs:
                z.fill_(77)
            chain.dispatch(dev(x), dev(res), *zs)
            return [host(z) for z in zs]
        want = run()
        accepted = set()
        for code in range(16):
            before = chain.tile()
            try:
                chain.set_tile(code)
            except L.SaberHipError:
                assert chain.tile() == before, (what, code)
                continue
            accepted.add(code)
            assert chain.tile() == code, (what, code)
            for g, w in zip(run(), want):
                assert np.array_equal(g, w), (what, code, "differs from code %d" % default)
        coop = accepted & {7, 15}
        assert (accepted - coop) == want_codes and coop in (set(), {7, 15} if what == "conv3x3+chain C=256" else set()), (what, sorted(accepted))

    forms = {64: {4, 2}, 128: {2, 1, 6, 5}}
    for Cc, H, Wd in ((64, 7, 9), (128, 5, 17), (256, 3, 5), (512, 3, 3)):
        K1 = 4 * Cc
        x = rng.integers(0, 256, (1, H, Wd, Cc)).astype(np.uint8)
        res = rng.integers(-128, 128, (1, H, Wd, K1)).astype(np.int8)
        ca = conv((1, Cc, H, Wd), K1, 1, 1, O.U8, O.S8, s_in, s_mid, 0, elt=True)
        cb = conv((1, K1, H, Wd), Cc, 1, 1, O.S8, O.U8, s_sum, s_out, 1)
        check("chain C=%d" % Cc, S.SaberConvChain(ca, cb), forms.get(Cc, {1, 9, 11} if Cc == 256 else {1, 9}), x, res, [ca, cb])
        if Cc == 512:
            continue
        c0 = conv((1, Cc, H, Wd), Cc, 3, 1, O.U8, O.U8, s_x, s_in, 1)
        check("conv3x3+chain C=%d" % Cc, S.SaberConvChain(ca, cb, conv3x3=c0), forms.get(Cc, {1, 3}), x, res, [ca, cb])
        check("conv3x3+conv1x1 C=%d" % Cc, S.SaberConvChain(ca, None, conv3x3=c0), forms.get(Cc, {1, 3}), x, res, [ca])
    for what, Cc, H, Wd, want_codes in (("strided head C=256", 256, 9, 7, {1, 3}), ("strided head + pair", 64, 27, 41, {4, 2})):
        K1 = 4 * Cc
        Ho, Wo = (H + 2 - 3) // 2 + 1, (Wd + 2 - 3) // 2 + 1
        Hs, Ws = 2 * Ho - (1 if H % 2 else 0), 2 * Wo - (1 if Wd % 2 else 0)
        x = rng.integers(0, 256, (1, H, Wd, Cc)).astype(np.uint8)
        res = rng.integers(-128, 128, (1, Hs, Ws, K1)).astype(np.int8)
        c0 = conv((1, Cc, H, Wd), Cc, 3, 2, O.U8, O.U8, s_x, s_in, 1)
        ca = conv((1, Cc, Ho, Wo), K1, 1, 1, O.U8, O.S8, s_in, s_mid, 0, elt=True, res_hw=(Hs, Ws))
        if Cc == 256:
            check(what, S.SaberConvChain(ca, None, conv3x3=c0), want_codes, x, res, [ca])
        else:
            pb = conv((1, K1, Ho, Wo), 512, 1, 1, O.S8, O.S8, s_sum, 0.045, 0)
            pc = conv((1, K1, Ho, Wo), 128, 1, 1, O.S8, O.U8, s_sum, 0.033, 1)
            check(what, S.SaberConvChain(ca, pb, conv3x3=c0, pair_b=pc), want_codes, x, res, [ca, pb, pc])


def _random_conv_geometry(rng, int8):
    k = int(rng.choice([1, 1, 3, 3, 3, 5, 7]))
    stride = int(rng.choice([1, 1, 1, 2]))
    dil = int(rng.choice([1, 1, 1, 2])) if k > 1 else 1
    pad = int(rng.choice([0, (dil * (k - 1)) // 2, (dil * (k - 1)) // 2, 1]))
    C = int(rng.choice([3, 4, 16, 32, 48, 64, 96, 128, 256, 512]) if int8 else rng.choice([3, 4, 8, 16, 32, 64, 96, 128, 256]))
    K = int(rng.choice([8, 10, 16, 24, 34, 40, 64, 72, 128, 200, 256]))
    N = int(rng.choice([1, 1, 2, 3, 8]))
    lo = dil * (k - 1) + 1 - 2 * pad
    H = int(rng.integers(max(lo, 1), 30))
    Wd = int(rng.integers(max(lo, 1), 34))
    if C >= 256 and k >= 5:
        k, pad, dil = 3, 1, 1
    return N, H, Wd, C, K, k, pad, stride, dil


# every kernel-selection code the library might accept for a conv: (tile | stage depth << 8 | variant << 16); refused ones are skipped
_I8_CODES = [t | (ks << 8) | (v << 16) for v in (1, 2, 3, 4) for t in range(6) for ks in (1, 2, 4)] + \
            [t | (ks << 8) | (v << 16) for v in (5, 6) for t in range(3) for ks in (1, 2, 4)] + [7 << 16, 8 << 16, 12 << 16] + \
            [rb | ((ib | nw) << 8) | (9 << 16) for rb in (1, 2, 4, 7) for ib in (1, 2) for nw in (0, 0x80)]
_F32_CODES = [t | ((ks | (sh << 4)) << 8) | (11 << 16) for t in range(10) for ks in (1, 2) for sh in (0, 1, 2, 3)] + \
             [v | (13 << 16) for v in range(1, 9)] + [v | (14 << 16) for v in range(0, 5)] + \
             [t | (ks << 8) | (v << 16) for v in (1, 2) for t in range(6) for ks in (1, 2, 4)]


@pytest.mark.parametrize("seed", range(40))
def test_conv_i8_random_geometry_every_accepted_selection_is_bit_exact(seed):
    """Property: for a random INT8 convolution (kernel 1 .. 7, stride, dilation, padding, ragged sizes, C from 3 to 512, any K, all input / output
    dtype combinations, relu or not) the static selection AND every kernel-selection code saber_hip_conv2d_set_tile accepts for it give the
    oracle's bytes. Shapes nobody picked by hand; 100 codes tried per case (implicit GEMM register / LDS-DMA forms, halo, image-resident, stem)."""
    rng = np.random.default_rng(9000 + seed)
    N, H, Wd, C, K, k, pad, stride, dil = _random_conv_geometry(rng, True)
    idt = int(rng.choice([O.S8, O.U8]))
    odt = int(rng.choice([O.S8, O.U8, O.F32]))
    relu = int(rng.integers(0, 2)) if odt != O.U8 else 1
    x = (rng.integers(0, 256, (N, H, Wd, C)).astype(np.uint8) if idt == O.U8 else rng.integers(-128, 128, (N, H, Wd, C)).astype(np.int8))
    w = (rng.standard_normal((K, C, k, k)) * np.sqrt(2.0 / (C * k * k))).astype(np.float32)
    b = (rng.standard_normal(K) * 0.5).astype(np.float32)
    in_scale, out_scale = float(rng.choice([0.017, 0.0039, 0.11])), float(rng.choice([0.041, 0.009, 0.3]))
    ws = O.weight_scales(w)
    wq = O.quant_weights(w, ws)
    bp, sc = O.conv_i8_prepare(ws, b, in_scale, out_scale, idt, odt)
    want = O.conv_i8(x, wq, bp, sc, odt, relu, (pad, pad), (stride, stride), (dil, dil))
    p = S.ConvParam(w, b, 1, (pad, pad), (stride, stride), (dil, dil), bool(relu), None)
    conv = S.SaberConv2D(int8=True).init((N, C, H, Wd), p, idt, odt, in_scale, out_scale)
    xin = dev(x)

    def run():
        y = conv.new_output()
        conv.dispatch(xin, y)
        return host(y)
    got = run()
    assert got.dtype == want.dtype and np.array_equal(got, want), ("static", conv.algo(), (N, H, Wd, C, K, k, pad, stride, dil))
    tried = set()
    for code in _I8_CODES:
        try:
            conv.set_tile(code)
        except L.SaberHipError:
            continue
        if conv.algo() in tried:
            continue
        tried.add(conv.algo())
        assert np.array_equal(run(), want), (conv.algo(), hex(code), (N, H, Wd, C, K, k, pad, stride, dil), idt, odt, relu)
    assert tried
    print("seed %d %s: %d kernel forms bit-exact" % (seed, (N, H, Wd, C, K, k, pad, stride, dil), len(tried)))


@pytest.mark.parametrize("seed", range(24))
def test_conv_f32_random_geometry_every_accepted_selection_within_tolerance(seed):
    """The FP32 twin: random geometry, optional in-place residual sum + relu, NHWC; the static selection and every accepted selection code (f32
    MFMA, bf16-plane implicit GEMM with its tiles / 8-wave forms / split-K, the halo and pointwise kernels) within 1e-4 of the oracle on both
    criteria, and the same bits on a second launch."""
    rng = np.random.default_rng(7000 + seed)
    N, H, Wd, C, K, k, pad, stride, dil = _random_conv_geometry(rng, False)
    elt = bool(rng.integers(0, 2))
    x = (rng.random((N, C, H, Wd)) * 3.0 - 1.0).astype(np.float32)
    w = (rng.standard_normal((K, C, k, k)) * np.sqrt(2.0 / (C * k * k))).astype(np.float32)
    b = (rng.standard_normal(K) * 0.5).astype(np.float32)
    want = O.conv_f32_nchw(x, w, b, not elt, (pad, pad), (stride, stride), (dil, dil))
    res = (rng.random(want.shape) * 2.0).astype(np.float32)
    if elt:
        want = np.maximum(want + res, 0.0)
    p = S.ConvParam(w, b, 1, (pad, pad), (stride, stride), (dil, dil), not elt)
    if elt:
        p.res_mode, p.res_relu, p.sum_scale = L.RES_SUM_INPLACE, True, 1.0
    conv = S.SaberConv2D(int8=False).init((N, C, H, Wd), p, L.F32, L.F32, in_layout=L.NHWC, out_layout=L.NHWC)
    xin = dev(np.ascontiguousarray(x.transpose(0, 2, 3, 1)))
    rin = np.ascontiguousarray(res.transpose(0, 2, 3, 1))

    def run():
        y = conv.new_output()
        if elt:
            y.copy_(dev(rin))
        conv.dispatch(xin, y)
        return host(y).transpose(0, 3, 1, 2)

    def check(what):
        got = run()
        d = np.abs(got - want)
        scale = max(float(np.abs(want).max()), 1e-6)
        e_max = float(d.max() / scale)
        e_el = float((d / (np.abs(want) + np.abs(want).mean() + 1e-12)).max())
        assert e_max <= FP32_RTOL and e_el <= FP32_RTOL, (what, conv.algo(), (N, H, Wd, C, K, k, pad, stride, dil), elt, e_max, e_el)
        assert np.array_equal(run(), got), ("not deterministic", conv.algo())
    check("static")
    tried = set()
    for code in _F32_CODES:
        try:
            conv.set_tile(code)
        except L.SaberHipError:
            continue
        if conv.algo() in tried:
            continue
        tried.add(conv.algo())
        check(hex(code))
    assert tried
    print("seed %d %s%s: %d kernel forms within 1e-4" % (seed, (N, H, Wd, C, K, k, pad, stride, dil), " + sum" if elt else "", len(tried)))


class StreamOp:
    """One launch of a streaming operator / fc / GEMM as the generators below yield it: run(T, ws=None) takes the device tensors by name
    (inputs; an output named in `oracle` is written in place when T has it, allocated by the wrapper otherwise) and returns {name: output
    tensor}; check(got, want) holds the operator's assertions on {name: ndarray}. prev: {name: ndarray} an in-place output starts from."""

    def __init__(self, name, run, check, ws_bytes=0, prev=None):
        self.name, self.run, self.check, self.ws_bytes, self.prev = name, run, check, ws_bytes, prev or {}


def run_stream_op(op, arrays, oracle):
    """the launch on ordinary tensors, outputs allocated by the wrappers (in-place ones start from op.prev); asserts op.check"""
    T = {n: dev(a) for n, a in arrays.items()}
    for n, a in op.prev.items():
        T[n] = dev(a.copy())
    got = op.run(T)
    op.check({n: host(got[n]) for n in oracle}, oracle)


def _fc_run(fc):
    def run(T, ws=None):
        if ws is not None:
            fc.ws = ws
        y = T["y"] if "y" in T else torch.empty((fc.desc.m, fc.desc.n), dtype=torch.float32, device="cuda")
        return {"y": fc.dispatch(T["x"], y)}
    return run


def _fc_ws(fc):
    return int(L.load().saber_hip_fc_workspace_bytes(fc.h))


def gen_pooling_eltwise_fc(seed):
    """test_pooling_eltwise_fc_random_shapes_vs_oracle's cases as (op, arrays, oracle) tuples, drawn in that test's order"""
    rng = np.random.default_rng(8800 + seed)
    # ---- pooling -----------------------------------------------------------------------------------------------------------------
    for _ in range(4):
        win = int(rng.integers(1, 6))
        st = int(rng.integers(1, 4))
        pad = int(rng.integers(0, (win + 1) // 2 + 0)) if win > 1 else 0
        pad = min(pad, win - 1)
        N, H, Wd, Cc = int(rng.integers(1, 4)), int(rng.integers(win, 40)), int(rng.integers(win, 40)), int(rng.choice([1, 3, 6, 10, 16, 24, 64, 100, 256]))
        pt = int(rng.integers(0, 3))
        floor = bool(rng.integers(0, 2))
        dt = int(rng.choice([O.S8, O.U8]))
        x = (rng.integers(0, 256, (N, H, Wd, Cc)).astype(np.uint8) if dt == O.U8 else rng.integers(-128, 128, (N, H, Wd, Cc)).astype(np.int8))
        want = O.pool_i8_nhwc(x, (win, win), (st, st), (pad, pad), pt, floor_mode=floor)
        geo = ((win, win), (st, st), (pad, pad), pt)

        def check_i8(got, w, what=("pool i8", (N, H, Wd, Cc), win, st, pad, pt, floor, dt)):
            assert got["y"].shape == w["y"].shape and np.array_equal(got["y"], w["y"]), what
        yield StreamOp("pooling_i8", lambda T, ws=None, g=geo, f=floor: {"y": S.pooling_i8(T["x"], *g, floor_mode=f, out=T.get("y"))}, check_i8), \
            {"x": x}, {"y": want}
        xf = rng.standard_normal((N, Cc, H, Wd)).astype(np.float32)
        wantf = O.pool_f32_nchw(xf, (win, win), (st, st), (pad, pad), pt, floor_mode=floor)

        # (a ceil-mode window that starts past the image - stride > window on the last row - averages nothing: NaN on both sides)
        def check_f(got, w, what=("pool f32", (N, Cc, H, Wd), win, st, pad, pt, floor)):
            assert np.array_equal(got["y"], w["y"], equal_nan=True), what
        yield StreamOp("pooling_f32_nchw", lambda T, ws=None, g=geo, f=floor: {"y": S.pooling_f32(T["x"], *g, floor_mode=f, out=T.get("y"))}, check_f), \
            {"x": xf}, {"y": wantf}
        xh = np.ascontiguousarray(xf.transpose(0, 2, 3, 1))
        yield StreamOp("pooling_f32_nhwc", lambda T, ws=None, g=geo, f=floor: {"y": S.pooling_f32(T["x"], *g, layout=L.NHWC, floor_mode=f, out=T.get("y"))},
                       check_f), {"x": xh}, {"y": np.ascontiguousarray(wantf.transpose(0, 2, 3, 1))}
    # ---- eltwise -----------------------------------------------------------------------------------------------------------------
    for _ in range(4):
        n = int(rng.choice([1, 15, 16, 17, 1003, 4096, 65537]))
        a, b = rng.integers(-128, 128, n).astype(np.int8), rng.integers(-128, 128, n).astype(np.int8)
        sa, sb = float(rng.uniform(0.01, 0.5)), float(rng.uniform(0.01, 0.5))
        c0, c1 = float(np.float32(rng.uniform(0.5, 20.0))), float(np.float32(rng.uniform(0.5, 20.0)))
        relu = bool(rng.integers(0, 2))

        def check_e(got, w, what=("eltwise", n, relu)):
            assert np.array_equal(got["y"], w["y"]), what
        yield StreamOp("eltwise_sum_i8", lambda T, ws=None, k=((c0, c1), relu, sa, sb): {"y": S.eltwise_sum(T["a"], T["b"], *k, out=T.get("y"))}, check_e), \
            {"a": a, "b": b}, {"y": O.eltwise_i8(a, b, sa, sb, c0, c1, relu)}
        fa, fb = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
        yield StreamOp("eltwise_sum_f32", lambda T, ws=None, k=((c0, c1), relu): {"y": S.eltwise_sum(T["a"], T["b"], *k, out=T.get("y"))}, check_e), \
            {"a": fa, "b": fb}, {"y": O.eltwise_f32(fa, fb, c0, c1, relu)}
    # ---- fully connected ---------------------------------------------------------------------------------------------------------
    for _ in range(3):
        M, N, K = int(rng.integers(1, 20)), int(rng.choice([1, 7, 10, 33, 64, 100, 1000])), int(rng.choice([16, 48, 100, 256, 528, 1000, 2048, 4112]))
        w = (rng.standard_normal((N, K)) * 0.05).astype(np.float32)
        b = rng.standard_normal(N).astype(np.float32)
        xf = rng.standard_normal((M, K)).astype(np.float32)
        want = O.fc_f32(xf, w, b)
        fc = S.SaberFc(False).init(M, N, K, w, b, L.F32)

        def check_fc32(got, wt, what=("fc f32", M, N, K, fc.algo())):
            assert np.abs(got["y"] - wt["y"]).max() <= FP32_RTOL * max(np.abs(wt["y"]).max(), 1e-6), what
        yield StreamOp("fc_f32:" + fc.algo(), _fc_run(fc), check_fc32, _fc_ws(fc)), {"x": xf}, {"y": want}
        if K % 16 == 0:
            ws = O.weight_scales(w)
            wq = O.quant_weights(w, ws)
            for dt in (L.S8, L.U8):
                xs = (rng.integers(0, 256, (M, K)).astype(np.uint8) if dt == L.U8 else rng.integers(-128, 128, (M, K)).astype(np.int8))
                fc = S.SaberFc(True).init(M, N, K, wq, b, dt, 0.031, 0.5 if dt == L.U8 else 1.0, w_scale=ws)
                wanti = O.fc_i8(xs, wq, ws, 0.031, b, 0.5) if dt == L.U8 else O.fc_i8(xs, wq, ws, 0.031, b)

                def check_fci(got, wt, what=("fc i8", M, N, K, dt, fc.algo())):
                    assert np.array_equal(got["y"], wt["y"]), what
                yield StreamOp("fc_i8:" + fc.algo(), _fc_run(fc), check_fci, _fc_ws(fc)), {"x": xs}, {"y": wanti}
            in_scale = float(np.abs(xf).max() / 127)
            fc = S.SaberFc(True).init(M, N, K, w, b, L.F32, in_scale)

            def check_fcq(got, wt, what=("fc i8 f32-in", M, N, K, fc.algo())):
                assert np.array_equal(got["y"], wt["y"]), what
            yield StreamOp("fc_i8_f32in:" + fc.algo(), _fc_run(fc), check_fcq, _fc_ws(fc)), {"x": xf}, \
                {"y": O.fc_i8(O.quant_flat_s8(xf, in_scale), wq, ws, in_scale, b)}


@pytest.mark.parametrize("seed", range(24))
def test_pooling_eltwise_fc_random_shapes_vs_oracle(seed):
    """The streaming operators on shapes drawn at random: 8-bit and FP32 pooling (window 1 .. 5, stride 1 .. 3, padding, ceil and floor output
    rule, max / the two averages, ragged sizes, channel counts that are not multiples of the vector width), INT8 and FP32 eltwise sums with
    arbitrary coefficients / scales / lengths, INT8 (s8 / u8 / quantise-on-entry) and FP32 fully connected layers with ragged M, N, K - the
    oracle's bytes where the path is integer or a fixed-order f32 reduction, 1e-4 for the FP32 fc. (The cases come from
    gen_pooling_eltwise_fc, which tests/test_gpu_guard.py runs again between guard bands.)"""
    ran = 0
    for op, arrays, oracle in gen_pooling_eltwise_fc(seed):
        run_stream_op(op, arrays, oracle)
        ran += 1
    assert ran >= 4 * 3 + 4 * 2 + 3


def gen_layout_quant_softmax_gemm(seed):
    """test_layout_quant_softmax_gemm_random_shapes_vs_oracle's cases as (op, arrays, oracle) tuples, drawn in that test's order"""
    rng = np.random.default_rng(6600 + seed)

    def eq(what):
        def check(got, w):
            assert np.array_equal(got["y"], w["y"]), what
        return check
    for _ in range(3):
        n, c, h, w = int(rng.integers(1, 4)), int(rng.choice([1, 3, 4, 5, 16, 17, 64, 100])), int(rng.integers(1, 30)), int(rng.integers(1, 30))
        x = (rng.standard_normal((n, c, h, w)) * 40.0).astype(np.float32)
        x.reshape(-1)[:: max(1, x.size // 50)] = np.float32(0.5) * np.round(x.reshape(-1)[:: max(1, x.size // 50)] * 2)      # exact .5 ties
        scale = float(rng.choice([0.25, 0.5, 1.0, 0.37]))
        for odt in (O.S8, O.U8):
            want = O.quant_nchw_to_nhwc(x, scale, odt)
            yield StreamOp("quantize_nchw_to_nhwc", lambda T, ws=None, k=(scale, odt): {"y": S.quantize_nchw_to_nhwc(T["x"], *k, out=T.get("y"))},
                           eq(("quantise", (n, c, h, w), scale, odt))), {"x": x}, {"y": want}
            yield StreamOp("dequantize_nhwc_to_nchw", lambda T, ws=None, k=scale: {"y": S.dequantize_nhwc_to_nchw(T["x"], k, out=T.get("y"))},
                           eq(("dequantise", (n, c, h, w), scale, odt))), {"x": want}, {"y": O.dequant_nhwc_to_nchw(want, scale)}
        c_pad = c + int(rng.integers(0, 4))
        t_ref = np.zeros((n, h, w, c_pad), np.float32)
        t_ref[..., :c] = x.transpose(0, 2, 3, 1)

        def check_t(got, wt, what=("nchw->nhwc", (n, c, h, w), c_pad), c=c):
            t = got["y"]
            assert np.array_equal(t[..., :c], wt["y"][..., :c]) and not t[..., c:].any(), what
        yield StreamOp("transpose_nchw_to_nhwc", lambda T, ws=None, k=c_pad: {"y": S.transpose_nchw_to_nhwc(T["x"], k, out=T.get("y"))}, check_t), \
            {"x": x}, {"y": t_ref}
        yield StreamOp("transpose_nhwc_to_nchw", lambda T, ws=None, k=c: {"y": S.transpose_nhwc_to_nchw(T["x"], k, out=T.get("y"))},
                       eq(("nhwc->nchw", (n, c, h, w), c_pad))), {"x": t_ref}, {"y": x}
        flat = (rng.standard_normal(int(rng.choice([1, 63, 64, 1000, 4097]))) * 30).astype(np.float32)
        yield StreamOp("quantize_flat_s8", lambda T, ws=None, k=scale: {"y": S.quantize_flat_s8(T["x"], k, out=T.get("y"))},
                       eq(("flat quantise", flat.size))), {"x": flat}, {"y": O.quant_flat_s8(flat, scale)}
    for _ in range(3):
        rows, cols = int(rng.integers(1, 20)), int(rng.choice([1, 2, 10, 63, 64, 65, 1000, 1001, 4096]))
        z = (rng.standard_normal((rows, cols)) * float(rng.choice([1.0, 10.0, 60.0]))).astype(np.float32)

        def check_s(got, wt, what=("softmax", rows, cols)):
            assert np.abs(got["y"] - wt["y"]).max() <= FP32_RTOL * wt["y"].max() and np.allclose(got["y"].sum(1), 1.0, atol=1e-5), what
        yield StreamOp("softmax", lambda T, ws=None: {"y": S.softmax(T["x"], out=T.get("y"))}, check_s), {"x": z}, {"y": O.softmax_f32(z)}
    for _ in range(3):
        M, N, K = int(rng.choice([1, 3, 8, 17, 64, 100])), int(rng.choice([1, 10, 64, 100, 1000])), int(rng.choice([1, 7, 64, 100, 513, 2048]))
        ta, tb = bool(rng.integers(0, 2)), bool(rng.integers(0, 2))
        alpha, beta = float(rng.choice([1.0, 0.5, -2.0])), float(rng.choice([0.0, 1.0, 0.25]))
        A = rng.standard_normal((K, M) if ta else (M, K)).astype(np.float32)
        Bm = rng.standard_normal((N, K) if tb else (K, N)).astype(np.float32)
        C0 = rng.standard_normal((M, N)).astype(np.float32)
        want = O.gemm_f32(A, Bm, M, N, K, ta, tb, alpha, beta, C0)

        def check_g(got, wt, what=("gemm", M, N, K, ta, tb, alpha, beta)):
            assert np.abs(got["c"] - wt["c"]).max() <= FP32_RTOL * max(np.abs(wt["c"]).max(), 1e-6), what
        yield StreamOp("gemm_f32", lambda T, ws=None, k=(ta, tb, M, N, K, alpha), be=beta: {"c": S.gemm(*k, T["a"], T["b"], be, T["c"])}, check_g,
                       prev={"c": C0}), {"a": A, "b": Bm}, {"c": want}


@pytest.mark.parametrize("seed", range(16))
def test_layout_quant_softmax_gemm_random_shapes_vs_oracle(seed):
    """The remaining operators of the path on shapes drawn at random: quantise f32 NCHW -> s8 / u8 NHWC (ties, saturation, channel padding),
    dequantise back, the two f32 transposes, flat quantisation, softmax over ragged row lengths (large logits included), Gemm with both
    transposes / alpha / beta on ragged M, N, K - bytes where the path is a rounding or a copy, 1e-4 for softmax and the GEMM. (The cases
    come from gen_layout_quant_softmax_gemm, which tests/test_gpu_guard.py runs again between guard bands.)"""
    ran = 0
    for op, arrays, oracle in gen_layout_quant_softmax_gemm(seed):
        run_stream_op(op, arrays, oracle)
        ran += 1
    assert ran == 3 * 7 + 3 + 3


RANDOM_FUSED_PAIRS = [None, (1.0, -0.5), (0.5, 1.0)]


@pytest.mark.parametrize("seed", range(16))
def test_conv_i8_fused_eltwise_random_geometry_every_accepted_selection(seed):
    """The executor's fused epilogue (conv -> s8, + residual x its scale, coefficients, optional relu, requantise: RES_ELTWISE) on random
    geometry: the oracle's conv followed by its SaberEltwise<AK_INT8>, byte for byte, under the static selection and every selection code
    set_tile accepts; and the in-place JIT sum (RES_JIT_SUM: conv accumulating onto the bytes already in the output) likewise."""
    rng = np.random.default_rng(9900 + seed)
    N, H, Wd, C, K, k, pad, stride, dil = _random_conv_geometry(rng, True)
    if C < 16:
        C = 16
    K = int(rng.choice([16, 32, 64, 128, 256]))
    idt = int(rng.choice([O.S8, O.U8]))
    relu = bool(rng.integers(0, 2))
    x = (rng.integers(0, 256, (N, H, Wd, C)).astype(np.uint8) if idt == O.U8 else rng.integers(-128, 128, (N, H, Wd, C)).astype(np.int8))
    w = (rng.standard_normal((K, C, k, k)) * np.sqrt(2.0 / (C * k * k))).astype(np.float32)
    b = (rng.standard_normal(K) * 0.5).astype(np.float32)
    in_scale, out_scale, s_res, s_out = 0.02, 0.05, float(rng.choice([0.043, 0.11])), float(rng.choice([0.06, 0.2]))
    c = float(np.float32(1.0 / s_out))
    ws = O.weight_scales(w)
    wq = O.quant_weights(w, ws)
    bp, sc = O.conv_i8_prepare(ws, b, in_scale, out_scale, idt, O.S8)
    y1 = O.conv_i8(x, wq, bp, sc, O.S8, 0, (pad, pad), (stride, stride), (dil, dil))
    res = rng.integers(-128, 128, y1.shape).astype(np.int8)
    pair = RANDOM_FUSED_PAIRS[seed % 3]         # per seed: the network's (c, c), (c, -c / 2), (c / 2, c)
    cc = _coeff_pair(c, pair)
    want = O.eltwise_i8(y1, res, out_scale, s_res, cc[0], cc[1], relu)
    if pair is not None:
        _coeff_conditions(y1, res, out_scale, s_res, cc, relu, "random geometry, seed %d %s" % (seed, pair))
    p = S.ConvParam(w, b, 1, (pad, pad), (stride, stride), (dil, dil), False, None)
    p.res_mode, p.res_relu, p.sum_scale, p.coeff, p.scale_res = L.RES_ELTWISE, relu, 1.0, cc, s_res
    conv = S.SaberConv2D(int8=True).init((N, C, H, Wd), p, idt, O.S8, in_scale, out_scale)
    xin, rd = dev(x), dev(res)

    def run():
        y = conv.new_output()
        conv.dispatch(xin, y, rd)
        return host(y)
    assert np.array_equal(run(), want), ("static", conv.algo(), (N, H, Wd, C, K, k, pad, stride, dil), idt, relu)
    tried = set()
    for code in _I8_CODES:
        try:
            conv.set_tile(code)
        except L.SaberHipError:
            continue
        if conv.algo() in tried:
            continue
        tried.add(conv.algo())
        assert np.array_equal(run(), want), (conv.algo(), hex(code), (N, H, Wd, C, K, k, pad, stride, dil), idt, relu)
    assert tried
