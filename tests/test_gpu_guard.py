"""Guard bands around every tensor of every launch form (tests/guard_util.py; tests/test_guard_cpu.py proves the harness on the CPU).

The other suites hand the library tensors from torch.empty: 512-byte aligned and followed by allocator slack (inside a Net: 256-byte arena
slots zeroed once). Here every tensor argument of a launch - inputs, residuals, every output, optional outputs, the in-place C of the GEMM -
sits in a buffer [1 MiB guard | 16 bytes | payload | 1 MiB guard]: aligned to 16 bytes and no more (the contract of include/saber_hip.h),
the guard starting at the very next byte, and the op's workspace is a guarded buffer full of the pattern. Per form, once per pattern
(0xFF: s8 -1 / f32 NaN; 0x5A: finite, large f32):

  (a) footprint     every guard of every tensor is intact after the launch, read-only tensors' and the workspace's included;
  (b) independence  the outputs under the two patterns and on ordinary tensors are byte-identical (FP32 too: the forms are deterministic);
  (c) value         the ordinary run equals the oracle under the criterion the op's own test uses (bytes for the integer paths, FP32_RTOL
                    on the two error measures for FP32); no stretch of the sentinel is left where the op defines the whole output.

What these tests cannot see: a load that is executed outside a tensor but whose value is discarded (it cannot be observed without
faulting), and an integer over-read that meets a zero weight (tests/test_guard_cpu.py states that limit). Library-owned buffers (packed
weights, padded bias / scale arrays, counters, split-K partials) are not guarded.

Forms are enumerated as the other suites do (their code lists, geometries and builders are imported, not copied); each test prints the
kernel names it ran and the closing test asserts that the names reached cover every form family."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from anakin_amd import lib as L  # noqa: E402
from anakin_amd import saber as S  # noqa: E402
from oracle import oracle as O  # noqa: E402
from tests import guard_util as GU  # noqa: E402
from tests import int8_probe as P  # noqa: E402
from tests import fp32_probe as FP  # noqa: E402
from tests import test_gpu_parity as TP  # noqa: E402
from tests import test_gpu_int8_probe as TI  # noqa: E402
from tests import test_gpu_fp32_probe as TF  # noqa: E402

FP32_RTOL = TP.FP32_RTOL
F32, S8, U8 = O.F32, O.S8, O.U8
NP_DT = {S8: np.int8, U8: np.uint8, F32: np.float32}

REACHED = {}            # family -> kernel names whose guarded launches ran and passed (a) and (b) in this session


@pytest.fixture(scope="module", autouse=True)
def _device():
    L.require_device()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bytes_of(t):
    return t.reshape(-1).view(torch.uint8)


def _plain(inputs, outputs, ws_bytes):
    """the same launch on ordinary tensors: dev(...) inputs, torch.empty outputs (sentinel or the previous bytes), torch.empty workspace"""
    T = {n: (None if a is None else dev(a)) for n, a in inputs.items()}
    for n, (shape, dt, prev) in outputs.items():
        t = torch.empty(tuple(shape), dtype=GU.torch_dtype(dt), device="cuda")
        if prev is None:
            _bytes_of(t).fill_(GU.SENTINEL)
        else:
            _bytes_of(t).copy_(_bytes_of(dev(prev)))
        T[n] = t
    return T, (torch.empty(max(int(ws_bytes), 16), dtype=torch.uint8, device="cuda") if ws_bytes else None)


def guard_launch(family, name, inputs, outputs, launch, ws_bytes=0, what=None):
    """One kernel form: ordinary tensors, then both guard patterns; asserts (a) and (b) and returns the ordinary run's outputs for (c).
    The name is recorded once the launches ran: the closing test asserts on what really ran."""
    got = GU.run_guarded(inputs, outputs, launch, "cuda", int(ws_bytes), plain=_plain, what=what or "%s: %s" % (family, name))
    torch.cuda.synchronize()
    REACHED.setdefault(family, set()).add(name)
    return got


def assert_bytes(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        i = tuple(int(v) for v in bad[0])
        raise AssertionError("%s: %d of %d values differ from the oracle, first at %s: got %s, oracle %s" % (what, len(bad), want.size, i, got[i], want[i]))


def assert_f32(got, want, what):
    """the two error measures of test_conv_f32_random_geometry_every_accepted_selection_within_tolerance"""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    d = np.abs(got - want)
    scale = max(float(np.abs(want).max()), 1e-6)
    e_max = float(d.max() / scale)
    e_el = float((d / (np.abs(want) + np.abs(want).mean() + 1e-12)).max())
    print("%s: e_max %.3g e_el %.3g" % (what, e_max, e_el))
    assert e_max <= FP32_RTOL and e_el <= FP32_RTOL, (what, e_max, e_el)        # (NaN fails both)


def _rand8(rng, shape, dt):
    return rng.integers(0, 256, shape).astype(np.uint8) if dt == U8 else rng.integers(-128, 128, shape).astype(np.int8)


def _nhwc(a):
    return np.ascontiguousarray(a.transpose(0, 2, 3, 1))


def _conv_ws(conv):
    return int(L.load().saber_hip_conv2d_workspace_bytes(conv.h))


def _conv_launch(conv):
    def launch(T, ws):
        if ws is not None:
            conv.ws = ws
        conv.dispatch(T["x"], T["y"], T.get("res"))
    return launch


# ==== INT8 convolution, every accepted form =================================================================================================
I8_EXTRA = {
    "m63": (1, 7, 9, 64, 72, 1, 0, 1),                # M = 63: one short of a tile
    "m162_c48_k34": (2, 9, 9, 48, 34, 3, 1, 1),       # M = 162, C % 64 != 0, K % 4 != 0
    "s2_13x11": (1, 13, 11, 32, 40, 3, 1, 2),
    "k5": (3, 5, 5, 16, 24, 5, 2, 1),
    "dil2": (1, 10, 10, 16, 16, 3, 2, 1, 2),
    "c3": (1, 9, 7, 3, 24, 3, 1, 1),                  # C < 4: padded through the workspace
}
I8_GEOS = dict(P.GEOMETRIES)
I8_GEOS.update(I8_EXTRA)
I8_MODES = {"u8u8": (U8, U8, 1), "s8s8": (S8, S8, 0), "u8f32": (U8, F32, 0), "elt": (U8, S8, 0), "sum": (U8, U8, 1)}
I8_CASES = [(g, m) for g in I8_GEOS for m in I8_MODES if I8_GEOS[g][3] >= 16 or m not in ("elt", "sum")] + [("c3", "f32in")]


def _i8_conv(geo, mode, seed):
    """(op, inputs, outputs, want()) of a random INT8 conv on geo in one of the modes; data and oracle as in
    test_conv_i8_random_geometry_... / test_conv_i8_fused_eltwise_random_geometry_... / test_conv_i8_jit_sum_inplace"""
    N, H, W, C, K, k, pad, stride, dil = geo if len(geo) == 9 else geo + (1,)
    rng = np.random.default_rng(seed)
    idt, odt, relu = I8_MODES.get(mode, (S8, U8, 1))
    w = (rng.standard_normal((K, C, k, k)) * np.sqrt(2.0 / (C * k * k))).astype(np.float32)
    b = (rng.standard_normal(K) * 0.5).astype(np.float32)
    in_scale, out_scale = 0.017, 0.041
    cp = S.ConvParam(w, b, 1, (pad, pad), (stride, stride), (dil, dil), bool(relu), None)
    kw = {}
    if mode == "f32in":
        xf = (rng.uniform(-1, 1, (N, C, H, W)) * 127 * in_scale).astype(np.float32)
        x, xq = xf, None
        kw = dict(in_layout=L.NCHW)
        idt_op = L.F32
    else:
        x = _rand8(rng, (N, H, W, C), idt)
        xq, idt_op = x, idt
    geo_o = (pad, pad), (stride, stride), (dil, dil)
    inputs, prev = {"x": x}, None
    s_res, s_out, ss = 0.043, 0.06, 0.61
    c = float(np.float32(1.0 / s_out))
    oh = (H + 2 * pad - dil * (k - 1) - 1) // stride + 1
    ow = (W + 2 * pad - dil * (k - 1) - 1) // stride + 1
    if mode == "elt":
        res = rng.integers(-128, 128, (N, oh, ow, K)).astype(np.int8)
        inputs["res"] = res
        cp.res_mode, cp.res_relu, cp.sum_scale, cp.coeff, cp.scale_res = L.RES_ELTWISE, True, 1.0, (c, c), s_res
    elif mode == "sum":
        prev = rng.integers(-128, 128, (N, oh, ow, K)).astype(np.int8)        # s8 bytes added into a u8 output
        cp.res_mode, cp.res_relu, cp.sum_scale, cp.res_dtype = L.RES_SUM_INPLACE, False, ss, S8
    conv = S.SaberConv2D(int8=True).init((N, C, H, W), cp, idt_op, odt, in_scale, out_scale, **kw)
    assert conv.out_shape() == (N, oh, ow, K), (conv.out_shape(), (N, oh, ow, K))

    def want():
        xs = O.quant_nchw_to_nhwc(x, in_scale, S8) if mode == "f32in" else xq
        ws = O.weight_scales(w)
        wq = O.quant_weights(w, ws)
        if mode == "elt":
            bp, sc = O.conv_i8_prepare(ws, b, in_scale, out_scale, idt, S8)
            return O.eltwise_i8(O.conv_i8(xs, wq, bp, sc, S8, 0, *geo_o), inputs["res"], out_scale, s_res, c, c, True)
        bp, sc = O.conv_i8_prepare(ws, b, in_scale, out_scale, O.code_of(xs), odt)
        if mode == "sum":
            rp = O.Residual(O.RES_JIT_SUM, 0, ss, S8, 0, 0, 0, 0)
            return O.conv_i8(xs, wq, bp, sc, odt, relu, *geo_o, residual=rp, out_init=prev.view(np.uint8))
        return O.conv_i8(xs, wq, bp, sc, odt, relu, *geo_o)
    outputs = {"y": ((N, oh, ow, K), NP_DT[odt], None if prev is None else prev.view(np.uint8))}
    return conv, inputs, outputs, want


def _run_conv_forms(family, what, conv, forms, inputs, outputs, want, check, launch=None, whole=True):
    """every (code, algo) of forms on one op: guard_launch + the value check against want() (computed once, on first need)"""
    ref, names = None, []
    launch = launch or _conv_launch(conv)
    for code, algo in forms:
        conv.set_tile(code)
        assert conv.algo() == algo, (conv.algo(), algo)
        got = guard_launch(family, algo, inputs, outputs, launch, _conv_ws(conv), "%s, %s (%s)" % (what, algo, hex(code)))
        names.append(algo)
        if ref is None:
            ref = want()
            ref = ref if isinstance(ref, dict) else {"y": ref}
        for n, r in ref.items():
            check(got[n], r, "%s, %s (%s), output '%s'" % (what, algo, hex(code), n))
            if whole and outputs[n][2] is None:
                GU.assert_no_sentinel_run(got[n], "%s, %s, output '%s'" % (what, algo, n))
    print("%s: %d kernel forms: %s" % (what, len(names), " ".join(names)))
    return names


@pytest.mark.parametrize("gname,mode", I8_CASES)
def test_conv_i8_every_accepted_form(gname, mode):
    """plain u8 -> u8 relu, s8 -> s8, u8 -> f32, fused eltwise with a guarded residual, in-place sum (s8 bytes under a u8 output), and the
    f32 NCHW image quantised on entry - on the probe geometries (K = 72 / 34 epilogues, image-resident forms, the stem) and on the shapes
    that are no whole tile; the static selection and every accepted code, one run per kernel name"""
    seed = 31000 + 97 * sorted(I8_GEOS).index(gname) + sorted(list(I8_MODES) + ["f32in"]).index(mode)
    conv, inputs, outputs, want = _i8_conv(I8_GEOS[gname], mode, seed)
    names = _run_conv_forms("conv_i8", "conv i8 %s %s %s" % (gname, I8_GEOS[gname], mode), conv, TI._forms(conv), inputs, outputs, want,
                            assert_bytes)          # (the f32 output too: test_conv_i8_random_geometry_... compares it for equality)
    assert names


def test_conv_i8_fused_eltwise_with_subsampled_residual():
    """test_conv_i8_fused_eltwise_with_subsampled_residual at (2, 15, 64, 128, 2): the shortcut is [n, 29, 29, k], read with stride 2"""
    n, ho, c, k, s = 2, 15, 64, 128, 2
    rng = np.random.default_rng(5 + ho + c)
    hs = ho * s - 1
    x = rng.integers(0, 256, (n, ho, ho, c)).astype(np.uint8)
    res_full = rng.integers(-128, 128, (n, hs, hs, k)).astype(np.int8)
    w = (rng.standard_normal((k, c, 1, 1)) * 0.05).astype(np.float32)
    b = (rng.standard_normal(k) * 0.2).astype(np.float32)
    in_scale, conv_scale, res_scale, out_scale = 0.02, 0.11, 0.09, 0.13
    coeff = 1.0 / out_scale
    p = S.ConvParam(w, b, 1, (0, 0), (1, 1), (1, 1), False)
    p.res_mode, p.res_relu, p.coeff, p.scale_res = L.RES_ELTWISE, True, (coeff, coeff), res_scale
    p.res_stride, p.res_hw = s, (hs, hs)
    conv = S.SaberConv2D(True).init((n, c, ho, ho), p, L.U8, L.S8, in_scale, conv_scale)

    def want():
        pooled = O.pool_i8_nhwc(res_full, (1, 1), (s, s), (0, 0), 0, floor_mode=True)
        ws = O.weight_scales(w)
        bp, sc = O.conv_i8_prepare(ws, b, in_scale, conv_scale, O.U8, O.S8)
        return O.eltwise_i8(O.conv_i8(x, O.quant_weights(w, ws), bp, sc, O.S8, 0, (0, 0)), pooled, conv_scale, res_scale, coeff, coeff, True)
    _run_conv_forms("conv_i8", "conv i8 + eltwise on a sub-sampled residual", conv, TI._forms(conv), {"x": x, "res": res_full},
                    {"y": ((n, ho, ho, k), np.int8, None)}, want, assert_bytes)


@pytest.mark.parametrize("hw", P.STEM_POOL_IMAGES)
@pytest.mark.parametrize("kind", ["u8", "s8", "f32"])
def test_stem_conv_maxpool_i8(hw, kind):
    """SaberConv2DPooling INT8: 7x7 / 2 stem + 3x3 / 2 max pooling in one launch (test_conv_pooling_stem_fused_vs_oracle's recipe)"""
    N, (H, W), K = 1, hw, 64
    rng = np.random.default_rng(H * 100 + W + len(kind))
    w = (rng.standard_normal((K, 3, 7, 7)) * 0.1).astype(np.float32)
    b = (rng.standard_normal(K) * 0.3).astype(np.float32)
    in_scale, out_scale, odt = 1 / 127.0, 0.02, (U8 if kind != "s8" else S8)
    if kind == "f32":
        x = rng.uniform(-1, 1, (N, 3, H, W)).astype(np.float32)
        idt, lay = L.F32, L.NCHW
    else:
        x = _rand8(rng, (N, H, W, 3), U8 if kind == "u8" else S8)
        idt, lay = O.code_of(x), L.NHWC
    cp = S.SaberConv2DPooling().init((N, 3, H, W), S.ConvParam(w, b, 1, (3, 3), (2, 2), (1, 1), odt == U8), L.POOL_MAX, (3, 3), (2, 2), (0, 0),
                                     idt, odt, in_scale, out_scale, in_layout=lay)
    assert cp.fused and "maxpool" in cp.algo(), cp.algo()           # (a fused conv + pooling has a single kernel: no other code is accepted)

    def want():
        xq = O.quant_nchw_to_nhwc(x, in_scale, S8) if kind == "f32" else x
        ws = O.weight_scales(w)
        bp, sc = O.conv_i8_prepare(ws, b, in_scale, out_scale, O.code_of(xq), odt)
        return O.pool_i8_nhwc(O.conv_i8(xq, O.quant_weights(w, ws), bp, sc, odt, odt == U8, (3, 3), (2, 2)), (3, 3), (2, 2), (0, 0), 0)

    def launch(T, ws):
        if ws is not None:
            cp.conv.ws = ws
        cp.dispatch(T["x"], T["y"])
    got = guard_launch("stem_pool_i8", cp.algo(), {"x": x}, {"y": (tuple(cp.new_output().shape), NP_DT[odt], None)}, launch, _conv_ws(cp.conv),
                       "stem + maxpool i8 %s %s, %s" % (hw, kind, cp.algo()))
    print("stem + maxpool i8 %s %s: %s" % (hw, kind, cp.algo()))
    assert_bytes(got["y"], want(), cp.algo())
    GU.assert_no_sentinel_run(got["y"], cp.algo())


@pytest.mark.parametrize("combo", [(S8, S8, 0), (U8, U8, 1)])
def test_image_resident_conv_with_fused_global_pooling(combo):
    """set_global_pooling on imgres1x1: the conv's bytes and their global average in one launch, both outputs guarded"""
    idt, odt, relu = combo
    N, H, W, C, K, k, pad, stride = P.GEOMETRIES["imgres1x1"]
    rng = np.random.default_rng(77 + idt)
    x = _rand8(rng, (N, H, W, C), idt)
    w = (rng.standard_normal((K, C, 1, 1)) * np.sqrt(2.0 / C)).astype(np.float32)
    b = (rng.standard_normal(K) * 0.5).astype(np.float32)
    conv = S.SaberConv2D(True).init((N, C, H, W), S.ConvParam(w, b, 1, (0, 0), (1, 1), (1, 1), bool(relu)), idt, odt, 0.03, 0.05)
    conv.set_tile(12 << 16)
    conv.set_global_pooling()
    assert conv.algo().endswith("+gpool"), conv.algo()

    def launch(T, ws):
        conv.dispatch_gpool(T["x"], T["y"], T["y_pool"])
    got = guard_launch("imgres", conv.algo(), {"x": x}, {"y": ((N, H, W, K), NP_DT[odt], None), "y_pool": ((N, 1, 1, K), NP_DT[odt], None)}, launch)
    print("gpool: %s" % conv.algo())
    ws = O.weight_scales(w)
    bp, sc = O.conv_i8_prepare(ws, b, 0.03, 0.05, idt, odt)
    want = O.conv_i8(x, O.quant_weights(w, ws), bp, sc, odt, relu)
    assert_bytes(got["y"], want, conv.algo())
    assert_bytes(got["y_pool"], O.pool_i8_nhwc(want, None, None, None, 1, global_pool=True).reshape(N, 1, 1, K), conv.algo() + " pooled")


# ==== FP32 convolution, every accepted form =================================================================================================
F32_GEOS = {n: FP.CONV_GEOMETRIES[n] for n in ("c48_k34", "c16_dil2", "stride2_13x11", "k5_nchw", "ragged_3x3", "ragged_1x1", "pw_c128_k512",
                                               "pw_c256_k64")}
F32_GEOS["res4_3x3_n8_cut"] = (8, 6, 7, 256, 256, 3, 1, 1, 1)          # FP.CONV_GEOMETRIES["res4_3x3_n8"] cut to 6x7: the split-K forms
assert FP.CONV_GEOMETRIES["res4_3x3_n8"][3:] == F32_GEOS["res4_3x3_n8_cut"][3:]
F32_NCHW_GEOS = {"nchw_c3": (2, 9, 7, 3, 24, 3, 1, 1, 1), "nchw_c6": (1, 6, 5, 6, 16, 3, 1, 1, 1)}      # transposed through the workspace, c_eff pads C
F32_CASES = [(g, "nhwc", e) for g in F32_GEOS for e in (False, True)] + [(g, "nchw", False) for g in F32_NCHW_GEOS]


def _f32_conv(geo, nchw, elt, seed):
    """test_conv_f32_random_geometry_...'s data: optional in-place residual sum + relu"""
    N, H, W, C, K, k, pad, stride, dil = geo
    rng = np.random.default_rng(seed)
    x = (rng.random((N, C, H, W)) * 3.0 - 1.0).astype(np.float32)
    w = (rng.standard_normal((K, C, k, k)) * np.sqrt(2.0 / (C * k * k))).astype(np.float32)
    b = (rng.standard_normal(K) * 0.5).astype(np.float32)
    p = S.ConvParam(w, b, 1, (pad, pad), (stride, stride), (dil, dil), not elt)
    if elt:
        p.res_mode, p.res_relu, p.sum_scale = L.RES_SUM_INPLACE, True, 1.0
    lay = L.NCHW if nchw else L.NHWC
    conv = S.SaberConv2D(int8=False).init((N, C, H, W), p, L.F32, L.F32, in_layout=lay, out_layout=lay)
    shape = conv.out_shape()
    res = (rng.random(shape) * 2.0).astype(np.float32) if elt else None

    def want():
        y = O.conv_f32_nchw(x, w, b, not elt, (pad, pad), (stride, stride), (dil, dil))
        y = y if nchw else _nhwc(y)
        return np.maximum(y + res, 0.0) if elt else y
    return conv, {"x": x if nchw else _nhwc(x)}, {"y": (shape, np.float32, res)}, want


@pytest.mark.parametrize("gname,layout,elt", F32_CASES)
def test_conv_f32_every_accepted_form(gname, layout, elt):
    """f32 MFMA, bf16-plane implicit GEMM (tiles, 8-wave forms, split-K), halo, pointwise and reduction-split kernels; NHWC in / out with and
    without the in-place residual sum + relu, NCHW in / out through the dirty workspace. Independence is exact: NaN guards, same bits."""
    geo = dict(F32_GEOS, **F32_NCHW_GEOS)[gname]
    conv, inputs, outputs, want = _f32_conv(geo, layout == "nchw", elt, 41000 + sorted(dict(F32_GEOS, **F32_NCHW_GEOS)).index(gname) * 2 + int(elt))
    names = _run_conv_forms("conv_f32", "conv f32 %s %s %s%s" % (gname, geo, layout, " + sum" if elt else ""), conv, TF._forms(conv), inputs,
                            outputs, want, assert_f32)
    assert names


@pytest.mark.parametrize("case", [(3, 8, 6, 10, 20, 1, 0), (2, 16, 12, 12, 32, 3, 1)])
def test_conv_f32_fused_relu_maxpool2x2(case):
    N, C, H, W, K, k, pad = case
    rng = np.random.default_rng(4300 + C + H)
    x = rng.standard_normal((N, H, W, C)).astype(np.float32)
    w = (rng.standard_normal((K, C, k, k)) * np.sqrt(2.0 / (C * k * k))).astype(np.float32)
    b = (rng.standard_normal(K) * 0.3).astype(np.float32)
    cp = S.SaberConv2DPooling(int8=False).init((N, C, H, W), S.ConvParam(w, b, 1, (pad, pad), (1, 1), (1, 1), True), 0, (2, 2), (2, 2), (0, 0),
                                                L.F32, L.F32)
    assert cp.fused and cp.algo().endswith("+maxpool2x2"), cp.algo()
    forms = TF._forms(cp.conv)
    assert all(a.endswith("+maxpool2x2") for _, a in forms), forms

    def launch(T, ws):
        if ws is not None:
            cp.conv.ws = ws
        cp.dispatch(T["x"], T["y"])

    def want():
        return _nhwc(O.pool_f32_nchw(O.conv_f32_nchw(np.ascontiguousarray(x.transpose(0, 3, 1, 2)), w, b, True, (pad, pad)), (2, 2), (2, 2), (0, 0), 0))
    _run_conv_forms("conv_f32_pool", "conv f32 + relu + maxpool2x2 %s" % (case,), cp.conv, forms, {"x": x},
                    {"y": (tuple(cp.new_output().shape), np.float32, None)}, want, assert_f32, launch=launch)


@pytest.mark.parametrize("case", [(1, 61, 47), (2, 33, 40)])
def test_stem_f32_one_launch(case):
    """conv_stem_f32.hip: NCHW image -> conv 7x7 / 2 + relu -> max pooling 3x3 / 2 -> NHWC in one launch, its four forms"""
    N, H, W = case
    rng = np.random.default_rng(900 + N + H + W)
    x = rng.uniform(-1, 1, (N, 3, H, W)).astype(np.float32)
    w = (rng.standard_normal((64, 3, 7, 7)) * np.sqrt(2.0 / 147)).astype(np.float32)
    b = (rng.standard_normal(64) * 0.2).astype(np.float32)
    stem = S.SaberConv2DPooling(int8=False).init((N, 3, H, W), S.ConvParam(w, b, 1, (3, 3), (2, 2), (1, 1), True), L.POOL_MAX, (3, 3), (2, 2), (0, 0),
                                                  L.F32, L.F32, in_layout=L.NCHW)
    assert stem.fused and stem.algo() == "stem7x7s2_maxpool3x3s2_f32_bf16x3_nchw_in", stem.algo()

    def launch(T, ws):
        if ws is not None:
            stem.conv.ws = ws
        stem.dispatch(T["x"], T["y"])
    ref = None
    for variant in (0, 1, 2, 3):
        stem.conv.set_tile((15 << 16) | variant)
        name = "%s/%d" % (stem.algo(), variant)
        got = guard_launch("stem_f32", name, {"x": x}, {"y": (tuple(stem.new_output().shape), np.float32, None)}, launch, _conv_ws(stem.conv))
        if ref is None:
            ref = _nhwc(O.pool_f32_nchw(O.conv_f32_nchw(x, w, b, True, (3, 3), (2, 2)), (3, 3), (2, 2), (0, 0), 0))
        assert_f32(got["y"], ref, name)
        GU.assert_no_sentinel_run(got["y"], name)
    print("stem f32 %s: forms 0..3 of %s" % (case, stem.algo()))


# ==== multi-tensor launches =================================================================================================================
from tests import dw_util as DU  # noqa: E402
from tests import sep_util as SU  # noqa: E402
from tests import test_gpu_dw as TD  # noqa: E402
from tests import test_gpu_group as TG  # noqa: E402
from tests import test_gpu_sep as TS  # noqa: E402
from tests import test_gpu_stage as TX  # noqa: E402
from tests import test_gpu_stage_tail as TT  # noqa: E402


class _QConv:
    """one INT8 conv op with random f32 weights and its oracle: ref(x[, res]) -> the oracle's bytes. elt = (res_relu, s_res, s_sum): fused
    eltwise (the conv requantises to s8 at s_out first); res_hw: the residual is [n, res_h, res_w, k], read with stride 2"""

    def __init__(self, rng, N, C, H, W, K, k, stride, idt, odt, s_in, s_out, relu, elt=None, res_hw=None):
        self.w = (rng.standard_normal((K, C, k, k)) * np.sqrt(2.0 / (k * k * C))).astype(np.float32)
        self.b = (rng.standard_normal(K) * 0.5).astype(np.float32)
        self.args = (k // 2, stride, idt, odt, s_in, s_out, relu, elt, res_hw)
        p = S.ConvParam(self.w, self.b, 1, (k // 2, k // 2), (stride, stride), (1, 1), bool(relu))
        if elt is not None:
            res_relu, s_res, s_sum = elt
            c = 1.0 / s_sum
            p.res_mode, p.res_relu, p.sum_scale, p.coeff, p.scale_res = L.RES_ELTWISE, bool(res_relu), 1.0, (c, c), s_res
            if res_hw is not None:
                p.res_stride, p.res_hw = 2, res_hw
        self.op = S.SaberConv2D(int8=True).init((N, C, H, W), p, idt, odt, s_in, s_out)
        self.shape = self.op.out_shape()
        self.np_dt = NP_DT[odt]

    def ref(self, x, res=None):
        pad, stride, idt, odt, s_in, s_out, relu, elt, res_hw = self.args
        ws = O.weight_scales(self.w)
        wq = O.quant_weights(self.w, ws)
        if elt is None:
            bp, sc = O.conv_i8_prepare(ws, self.b, s_in, s_out, idt, odt)
            return O.conv_i8(x, wq, bp, sc, odt, int(relu), (pad, pad), (stride, stride))
        res_relu, s_res, s_sum = elt
        c = 1.0 / s_sum
        bp, sc = O.conv_i8_prepare(ws, self.b, s_in, s_out, idt, S8)
        t = O.conv_i8(x, wq, bp, sc, S8, 0, (pad, pad), (stride, stride))
        if res_hw is not None:
            res = O.pool_i8_nhwc(res, (1, 1), (2, 2), (0, 0), 0, floor_mode=True)
        return O.eltwise_i8(t, res, s_out, s_res, c, c, bool(res_relu))


_S = dict(s_x=0.023, s_in=0.02, s_mid=0.05, s_res=0.043, s_sum=0.06, s_out=0.031)      # the chain tests' scales


def _out(q):
    return (q.shape, q.np_dt, None)


def _check_outputs(got, wants, what):
    for n, w in wants.items():
        assert_bytes(got[n], w, "%s, output '%s'" % (what, n))
        GU.assert_no_sentinel_run(got[n], "%s, output '%s'" % (what, n))


def _chain_codes(chain):
    """[code]: the default form first, then every other code 0..15 the chain accepts (restores the default)"""
    default = chain.tile()
    codes = [default]
    for code in range(16):
        try:
            chain.set_tile(code)
        except L.SaberHipError:
            continue
        if code != default:
            codes.append(code)
    chain.set_tile(default)
    return codes


def _run_chain(family, what, chain, inputs, outs, wants_fn):
    """every accepted form of one chain object (the cooperative forms keep their counters: all runs on this object)"""
    def launch(T, ws):
        chain.dispatch(T["x"], T["res"], *[T[n] for n in outs])
    wants, names = None, []
    for code in _chain_codes(chain):
        chain.set_tile(code)
        name = "%s/form%d" % (what.split(" @")[0], code)
        got = guard_launch(family, name, inputs, outs, launch, 0, "%s, chain form %d" % (what, code))
        names.append(name)
        wants = wants or wants_fn()
        _check_outputs(got, wants, "%s, chain form %d" % (what, code))
    print("%s: forms %s" % (what, " ".join(n.rsplit("/", 1)[1] for n in names)))


def test_conv_i8_sibling_pair():
    """two INT8 convs over one input in one launch at the probe suite's PAIR_GEO, s8 and u8 on either side, every accepted form"""
    N, H, W, C, K1, K2, k, pad, stride = TI.PAIR_GEO
    rng = np.random.default_rng(5101)
    for idt in (U8, S8):
        x = _rand8(rng, (N, H, W, C), idt)
        a = _QConv(rng, N, C, H, W, K1, k, stride, idt, S8, 0.02, 0.05, 0)
        b = _QConv(rng, N, C, H, W, K2, k, stride, idt, U8, 0.02, 0.033, 1)
        pair = S.SaberConvPair(a.op, b.op)
        wants = None

        def launch(T, ws):
            pair.dispatch(T["x"], T["ya"], T["yb"])
        for code, algo in TI._forms(pair):
            pair.set_tile(code)
            got = guard_launch("pair_i8", algo, {"x": x}, {"ya": _out(a), "yb": _out(b)}, launch, 0, "pair i8 %s (%s)" % (algo, hex(code)))
            wants = wants or {"ya": a.ref(x), "yb": b.ref(x)}
            _check_outputs(got, wants, "pair i8 %s" % algo)
    print("pair i8: %s" % " ".join(sorted(REACHED["pair_i8"])))


# the selection codes test_conv_f32_sibling_pair_equals_two_ops runs a pair through (tile | stage depth << 8 | variant << 16)
F32_PAIR_CODES = [0 | (1 << 8) | (1 << 16), 2 | (2 << 8) | (1 << 16), 3 | (4 << 8) | (1 << 16), 5 | (1 << 8) | (1 << 16), 2 | (4 << 8) | (2 << 16),
                  1 | (4 << 8) | (3 << 16), 0 | (4 << 8) | (4 << 16)]


def test_conv_f32_sibling_pair():
    N, H, W, C, K1, K2, k, pad, stride = (1, 6, 6, 32, 128, 16, 3, 1, 1)
    assert (N, H, W, C, K1, K2, k, pad, stride) in FP.PAIR_GEOMETRIES
    rng = np.random.default_rng(5102)
    x = rng.standard_normal((N, H, W, C)).astype(np.float32)
    convs, ws_, bs = [], [], []
    for K, relu in ((K1, False), (K2, True)):
        w = (rng.standard_normal((K, C, k, k)) * np.sqrt(2.0 / (C * k * k))).astype(np.float32)
        b = (rng.standard_normal(K) * 0.5).astype(np.float32)
        ws_.append(w)
        bs.append(b)
        convs.append(S.SaberConv2D(False).init((N, C, H, W), S.ConvParam(w, b, 1, (pad, pad), (stride, stride), (1, 1), relu), L.F32, L.F32,
                                               in_layout=L.NHWC, out_layout=L.NHWC))
    pair = S.SaberConvPair(convs[0], convs[1])
    assert pair.algo().startswith("pair_igemm_f32"), pair.algo()

    def launch(T, ws):
        pair.dispatch(T["x"], T["ya"], T["yb"])
    wants = None
    forms = [(L.load().saber_hip_conv2d_get_tile(pair.h), pair.algo())]
    for code in F32_PAIR_CODES:
        try:
            pair.set_tile(code)
        except L.SaberHipError:
            continue
        if pair.algo() not in [a for _, a in forms]:
            forms.append((code, pair.algo()))
    for code, algo in forms:
        pair.set_tile(code)
        got = guard_launch("pair_f32", algo, {"x": x}, {"ya": (convs[0].out_shape(), np.float32, None), "yb": (convs[1].out_shape(), np.float32, None)},
                           launch, 0, "pair f32 %s (%s)" % (algo, hex(code)))
        xn = np.ascontiguousarray(x.transpose(0, 3, 1, 2))
        wants = wants or [_nhwc(O.conv_f32_nchw(xn, ws_[i], bs[i], bool(i), (pad, pad), (stride, stride))) for i in (0, 1)]
        for n, wnt in zip(("ya", "yb"), wants):
            assert np.abs(got[n] - wnt).max() <= FP32_RTOL * np.abs(wnt).max(), (algo, n)       # (the pair test's criterion)
            GU.assert_no_sentinel_run(got[n], "pair f32 %s %s" % (algo, n))
    print("pair f32: %s" % " ".join(a for _, a in forms))


CHAIN_SHAPES = [(64, 7, 9), (128, 5, 17), (256, 3, 5), (512, 3, 3)]


@pytest.mark.parametrize("shape", CHAIN_SHAPES)
def test_conv_chains(shape):
    """[1x1 + eltwise] -> 1x1, and 3x3 -> [1x1 + eltwise] (-> 1x1) in one launch: every code 0..15 each kind of chain accepts"""
    Cc, H, W = shape
    K1 = 4 * Cc
    rng = np.random.default_rng(5200 + Cc)
    x = _rand8(rng, (1, H, W, Cc), U8)
    res = rng.integers(-128, 128, (1, H, W, K1)).astype(np.int8)
    c0 = _QConv(rng, 1, Cc, H, W, Cc, 3, 1, U8, U8, _S["s_x"], _S["s_in"], 1) if Cc != 512 else None
    ca = _QConv(rng, 1, Cc, H, W, K1, 1, 1, U8, S8, _S["s_in"], _S["s_mid"], 0, elt=(1, _S["s_res"], _S["s_sum"]))
    cb = _QConv(rng, 1, K1, H, W, Cc, 1, 1, S8, U8, _S["s_sum"], _S["s_out"], 1)

    def wants(x_in):
        y1 = ca.ref(x_in, res)
        return {"y1": y1, "y2": cb.ref(y1)}
    _run_chain("chain1x1", "chain1x1_c%d @%s" % (Cc, shape), S.SaberConvChain(ca.op, cb.op), {"x": x, "res": res}, {"y1": _out(ca), "y2": _out(cb)},
               lambda: wants(x))
    if c0 is None:
        return
    _run_chain("chain3x3", "chain3x3_c%d @%s" % (Cc, shape), S.SaberConvChain(ca.op, cb.op, conv3x3=c0.op), {"x": x, "res": res},
               {"y1": _out(ca), "y2": _out(cb)}, lambda: wants(c0.ref(x)))
    _run_chain("chain3x3", "chain3x3_no_second_c%d @%s" % (Cc, shape), S.SaberConvChain(ca.op, None, conv3x3=c0.op), {"x": x, "res": res},
               {"y1": _out(ca)}, lambda: {"y1": ca.ref(c0.ref(x), res)})


@pytest.mark.parametrize("shape", [(256, 9, 7), (64, 27, 41)])
def test_strided_head_chains(shape):
    """3x3 / stride 2 -> [1x1 + eltwise on the shortcut sub-sampled by 2], and at C = 64 the same with the next stage's sibling pair"""
    Cc, H, W = shape
    K1 = 4 * Cc
    rng = np.random.default_rng(5300 + Cc)
    Ho, Wo = (H + 2 - 3) // 2 + 1, (W + 2 - 3) // 2 + 1
    Hs, Ws = 2 * Ho - (1 if H % 2 else 0), 2 * Wo - (1 if W % 2 else 0)
    x = _rand8(rng, (1, H, W, Cc), U8)
    res = rng.integers(-128, 128, (1, Hs, Ws, K1)).astype(np.int8)
    c0 = _QConv(rng, 1, Cc, H, W, Cc, 3, 2, U8, U8, _S["s_x"], _S["s_in"], 1)
    ca = _QConv(rng, 1, Cc, Ho, Wo, K1, 1, 1, U8, S8, _S["s_in"], _S["s_mid"], 0, elt=(1, _S["s_res"], _S["s_sum"]), res_hw=(Hs, Ws))
    _run_chain("head", "head_c%d @%s" % (Cc, shape), S.SaberConvChain(ca.op, None, conv3x3=c0.op), {"x": x, "res": res}, {"y1": _out(ca)},
               lambda: {"y1": ca.ref(c0.ref(x), res)})
    if Cc != 64:
        return                                         # (the head with the pair exists at C = 64: 640 channels in all)
    pb = _QConv(rng, 1, K1, Ho, Wo, 512, 1, 1, S8, S8, _S["s_sum"], 0.045, 0)
    pc = _QConv(rng, 1, K1, Ho, Wo, 128, 1, 1, S8, U8, _S["s_sum"], 0.033, 1)

    def wants():
        y1 = ca.ref(c0.ref(x), res)
        return {"y1": y1, "yb": pb.ref(y1), "yc": pc.ref(y1)}
    _run_chain("head", "head_pair_c%d @%s" % (Cc, shape), S.SaberConvChain(ca.op, pb.op, conv3x3=c0.op, pair_b=pc.op), {"x": x, "res": res},
               {"y1": _out(ca), "yb": _out(pb), "yc": _out(pc)}, wants)


@pytest.mark.parametrize("hw", [(18, 23), (30, 30)])
@pytest.mark.parametrize("kind", ["f32", "u8"])
def test_stem_pair(hw, kind):
    """stem conv + max pooling + the two 1x1 convs reading the pooled tensor in one launch, y_pool present and absent"""
    N, (H, W) = 1, hw
    rng = np.random.default_rng(5400 + H + len(kind))
    w = (rng.standard_normal((64, 3, 7, 7)) * 0.1).astype(np.float32)
    b = (rng.standard_normal(64) * 0.3).astype(np.float32)
    in_scale, pool_scale, odt = 1 / 127.0, 0.02, U8
    if kind == "f32":
        x = rng.uniform(-1, 1, (N, 3, H, W)).astype(np.float32)
        idt, lay = L.F32, L.NCHW
    else:
        x = _rand8(rng, (N, H, W, 3), U8)
        idt, lay = U8, L.NHWC
    stem = S.SaberConv2DPooling().init((N, 3, H, W), S.ConvParam(w, b, 1, (3, 3), (2, 2), (1, 1), True), L.POOL_MAX, (3, 3), (2, 2), (0, 0), idt, odt,
                                       in_scale, pool_scale, in_layout=lay)
    assert stem.fused
    pshape = tuple(stem.new_output().shape)
    ph, pw = pshape[1:3]
    qa = _QConv(rng, N, 64, ph, pw, 256, 1, 1, odt, S8, pool_scale, 0.05, 0)
    qb = _QConv(rng, N, 64, ph, pw, 64, 1, 1, odt, U8, pool_scale, 0.031, 1)
    sp = S.SaberStemPair(stem, qa.op, qb.op)
    name = "stem_pair/" + stem.algo()

    def launch(T, ws):
        if ws is not None:
            stem.conv.ws = ws
        sp.dispatch(T["x"], T["ya"], T["yb"], T.get("y_pool"))
    wants = None
    for with_pool in (True, False):
        outs = {"ya": _out(qa), "yb": _out(qb)}
        if with_pool:
            outs["y_pool"] = (pshape, np.uint8, None)
        got = guard_launch("stem_pair", name + ("+y_pool" if with_pool else ""), {"x": x}, outs, launch, _conv_ws(stem.conv))
        if wants is None:
            xq = O.quant_nchw_to_nhwc(x, in_scale, S8) if kind == "f32" else x
            ws_ = O.weight_scales(w)
            bp, sc = O.conv_i8_prepare(ws_, b, in_scale, pool_scale, O.code_of(xq), odt)
            pooled = O.pool_i8_nhwc(O.conv_i8(xq, O.quant_weights(w, ws_), bp, sc, odt, 1, (3, 3), (2, 2)), (3, 3), (2, 2), (0, 0), 0)
            wants = {"ya": qa.ref(pooled), "yb": qb.ref(pooled), "y_pool": pooled}
        _check_outputs(got, {n: wants[n] for n in outs}, name)
    print("stem pair %s %s: %s" % (hw, kind, name))


def _stage_tensors(ops, tail_op=None):
    outs = {}
    for k, (c0, ca, cb) in enumerate(ops):
        outs["y1_%d" % k] = (ca.out_shape(), NP_DT[ca.desc.out_dtype], None)
        outs["y2_%d" % k] = (cb.out_shape(), NP_DT[cb.desc.out_dtype], None)
    if tail_op is not None:
        outs["y_tail"] = (tail_op.out_shape(), np.int8, None)
    return outs


@pytest.mark.parametrize("shape", [(256, 2, 7, 9, 2), (128, 1, 5, 13, 2), (64, 2, 7, 9, 3)])
def test_chain_stage(shape):
    """a run of 3x3-led chains as one persistent launch (conv_stage_coop.hip): the same object for every run - its counters run on.
    C = 64 (conv_stage1_c64_kernel; three blocks whose hand-over dtype alternates) also in the form with the inner blocks' y1 pointers
    null: the inner tensors stay guarded tensors the launch is not given, and come back sentinel throughout"""
    Cc, N, H, W, nblk = shape
    rng = np.random.default_rng(4100 + N + H + nblk + Cc)
    x, res, ops, wants = TP._res4_blocks(rng, N, H, W, nblk, Cc=Cc)
    chains = [S.SaberConvChain(ca, cb, conv3x3=c0) for c0, ca, cb in ops]
    stage = S.SaberChainStage(chains)
    outs = _stage_tensors(ops)
    for skip in ((), range(nblk - 1)) if Cc == 64 else ((),):
        def launch(T, ws):
            stage.dispatch(T["x"], T["res"], [None if k in skip else T["y1_%d" % k] for k in range(nblk)], [T["y2_%d" % k] for k in range(nblk)])
        name = "stage_c%d" % Cc + ("_inner_y1_null" if skip else "")
        got = guard_launch("stage", name, {"x": x, "res": res}, outs, launch)
        print("chain stage %s: %s" % (shape, name))
        for k in skip:
            y = got.pop("y1_%d" % k).view(np.uint8)
            assert (y == GU.SENTINEL).all(), "%s: the y1 of block %d the launch was not given was written: %d bytes" % (name, k, int((y != GU.SENTINEL).sum()))
        _check_outputs(got, {n: wants[int(n[3:])][int(n[1]) - 1] for n in got}, name)


@pytest.mark.parametrize("case", TT.TAIL_CASES[:2])
def test_chain_stage_with_tail(case):
    """the res4 stage launch with the strided head as its tail: every block's two outputs and the tail's output guarded"""
    N, H, W, nblk, mdt, res_relu = case
    rng = np.random.default_rng(7300 + N + H + nblk)
    x, res, ops, wants = TT._res4_blocks(rng, N, H, W, nblk)
    last_dt = U8 if (nblk - 1) % 2 == 0 else S8
    c3t, cat, want_t = TT._head(rng, N, H, W, last_dt, mdt, res_relu, x_in=wants[-1][1], res_in=wants[-1][0])
    chains = [S.SaberConvChain(ca, cb, conv3x3=c0) for c0, ca, cb in ops]
    tail = S.SaberConvChain(cat, None, conv3x3=c3t)
    stage = S.SaberChainStage(chains, tail=tail)
    outs = _stage_tensors(ops, cat)

    def launch(T, ws):
        stage.dispatch(T["x"], T["res"], [T["y1_%d" % k] for k in range(nblk)], [T["y2_%d" % k] for k in range(nblk)], T["y_tail"])
    got = guard_launch("tail", "stage_c256+tail", {"x": x, "res": res}, outs, launch)
    print("chain stage with tail %s" % (case,))
    w = {"y%d_%d" % (j + 1, k): wants[k][j] for k in range(nblk) for j in (0, 1)}
    w["y_tail"] = want_t
    _check_outputs(got, w, "stage + tail")


@pytest.mark.parametrize("N", [1, 3])
def test_xcd_stage_res5(N):
    """the XCD-resident stage (stage_xcd.hip): res5's ten convolutions on 7x7 images as one persistent launch, every slot guarded; the value
    reference is the ops dispatched one by one, as in tests/test_gpu_stage.py (each is pinned to the oracle by the parity tests)"""
    rng = np.random.default_rng(900 + N)
    ph, nt = TX.res5(rng, N)
    x0 = rng.integers(-128, 128, (N, 7, 7, 1024)).astype(np.int8)
    stage = S.SaberStage(ph)
    outs = {"t%d" % o: (c.out_shape(), NP_DT[c.desc.out_dtype], None) for c, i, o, r in ph}

    def launch(T, ws):
        stage.dispatch([T["x"]] + [T["t%d" % k] for k in range(1, nt)])
        stage.status()
    got = guard_launch("xcd_stage", "stage_xcd_res5", {"x": x0}, outs, launch)
    print("XCD stage res5 N=%d: %d phases" % (N, len(ph)))
    want = [dev(x0)] + [None] * (nt - 1)
    for c, i, o, r in ph:
        want[o] = c.new_output()
        c.dispatch(want[i], want[o], None if r < 0 else want[r])
    torch.cuda.synchronize()
    _check_outputs(got, {"t%d" % k: want[k].cpu().numpy() for k in range(1, nt)}, "XCD stage")


@pytest.mark.parametrize("case", TX.IMG_CASES)
def test_image_resident_variant_12(case):
    """kernel variant 12 (one workgroup = one image x a channel group) at (1, 5, 6): 30 pixels, ragged"""
    cin, cout, k, relu, idt, odt, elt = case
    N, H, W = 1, 5, 6
    rng = np.random.default_rng(cin + cout + N)
    q = _QConv(rng, N, cin, H, W, cout, k, 1, idt, odt, 0.03, 0.05, relu, elt=(1, 0.04, 0.05) if elt else None)
    x = _rand8(rng, (N, H, W, cin), idt)
    res = rng.integers(-128, 128, (N, H, W, cout)).astype(np.int8) if elt else None
    q.op.set_tile(12 << 16)
    assert q.op.algo().startswith("imgres"), q.op.algo()
    got = guard_launch("imgres", q.op.algo(), {"x": x, "res": res}, {"y": _out(q)}, _conv_launch(q.op), _conv_ws(q.op))
    print("image-resident: %s" % q.op.algo())
    _check_outputs(got, {"y": q.ref(x, res)}, q.op.algo())


@pytest.mark.parametrize("gi", range(4))
def test_separable_pairs(gi):
    """depthwise 3x3 + pointwise 1x1 in one launch on SU.GEOMETRIES[0..3]: every code, y_dw present and absent"""
    names = []
    for di in (0, 1):
        cs = SU.case(gi, di)
        dw, pw = TS.make_pair(cs.geo, cs.dts, cs.w_dw, cs.b_dw, None, cs.w_pw, cs.b_pw, None, SU.IN_SCALE, cs.mid_scale, cs.out_scale)
        sep = S.SaberConvSep(dw, pw)

        def launch(T, ws):
            sep.dispatch(T["x"], T["y_pw"], T.get("y_dw"))
        for code in TS.forms_of(sep):
            sep.set_tile(code)
            for with_dw in (True, False):
                outs = {"y_pw": (pw.out_shape(), NP_DT[cs.dts[2]], None)}
                if with_dw:
                    outs["y_dw"] = (dw.out_shape(), NP_DT[cs.dts[1]], None)
                got = guard_launch("sep", sep.algo(), {"x": cs.x}, outs, launch, 0, "sep %s %s code %d%s" % (cs.geo, sep.algo(), code, "" if with_dw else ", no y_dw"))
                _check_outputs(got, {"y_pw": cs.out, "y_dw": cs.mid} if with_dw else {"y_pw": cs.out}, sep.algo())
            names.append(sep.algo())
    assert names
    print("sep %s: %s" % (SU.GEOMETRIES[gi], " ".join(sorted(set(names)))))


@pytest.mark.parametrize("gname", sorted(P.DW_GEOMETRIES))
def test_depthwise_forms(gname):
    """depthwise 3x3, INT8 and FP32, on DW_GEOMETRIES: the static choice, the direct kernel and every depthwise form"""
    N, H, W, C, K, k, pad, stride = P.DW_GEOMETRIES[gname]
    rng = np.random.default_rng(5500 + stride)
    for in_dt, out_dt, relu in ((U8, U8, True), (S8, S8, False)):
        conv, xt, want, _ = TD._i8_case(rng, N, C, H, W, stride, pad, in_dt, out_dt, relu, True)
        x = xt.cpu().numpy()
        for label, code in TD._selections(conv):
            if code is not None:
                conv.set_tile(code)
            got = guard_launch("dw", conv.algo(), {"x": x}, {"y": (conv.out_shape(), NP_DT[out_dt], None)}, _conv_launch(conv), _conv_ws(conv))
            _check_outputs(got, {"y": want}, "dw i8 %s %s" % (label, conv.algo()))
    x = rng.standard_normal((N, C, H, W)).astype(np.float32)
    wt = (rng.standard_normal((C, 1, 3, 3)) * np.sqrt(2.0 / 9)).astype(np.float32)
    b = (rng.standard_normal(C) * 0.3).astype(np.float32)
    conv = S.SaberConv2D(False).init((N, C, H, W), S.ConvParam(wt, b, C, (pad, pad), (stride, stride), (1, 1), True), L.F32, L.F32,
                                     in_layout=L.NHWC, out_layout=L.NHWC)
    want = None
    for label, code in TD._selections(conv):
        if code is not None:
            conv.set_tile(code)
        got = guard_launch("dw", conv.algo(), {"x": _nhwc(x)}, {"y": (conv.out_shape(), np.float32, None)}, _conv_launch(conv), _conv_ws(conv))
        want = want if want is not None else _nhwc(O.conv_f32_nchw(x, wt, b, True, (pad, pad), (stride, stride), group=C))
        assert_f32(got["y"], want, "dw f32 %s %s" % (label, conv.algo()))
        GU.assert_no_sentinel_run(got["y"], conv.algo())
    print("depthwise %s: %s" % (gname, " ".join(sorted(REACHED["dw"]))))


@pytest.mark.parametrize("cg", [4, 32])
def test_grouped_3x3_forms(cg):
    """the grouped 3x3 INT8 form (variant 17) at C = 64, odd H / W, stride 1 and 2, pad 0 and 1"""
    rng = np.random.default_rng(5600 + cg)
    for (h, w, s, p), (in_dt, out_dt, relu) in zip(((7, 9, 1, 1), (9, 7, 2, 1), (5, 11, 1, 0), (11, 5, 2, 0)),
                                                    ((U8, U8, True), (S8, S8, False), (U8, S8, False), (S8, U8, True))):
        conv, xt, want, _ = TG._i8_case(rng, 2, 64, cg, h, w, s, p, in_dt, out_dt, relu, True)
        x = xt.cpu().numpy()
        for label, code in TG._selections(conv):
            if code is not None:
                conv.set_tile(code)
            got = guard_launch("group", conv.algo(), {"x": x}, {"y": (conv.out_shape(), NP_DT[out_dt], None)}, _conv_launch(conv), _conv_ws(conv),
                               "group Cg=%d %s %s %s" % (cg, (h, w, s, p), label, conv.algo()))
            _check_outputs(got, {"y": want}, "group Cg=%d %s %s" % (cg, (h, w, s, p), conv.algo()))
    print("grouped Cg=%d: %s" % (cg, " ".join(sorted(REACHED["group"]))))


# ==== streaming ops, fc and GEMM ============================================================================================================
def _guard_stream(family, op, arrays, oracle, what):
    """a StreamOp of tests/test_gpu_parity.py between guard bands: (a), (b), then the operator's own assertions on the ordinary run"""
    outs = {n: (w.shape, w.dtype, op.prev.get(n)) for n, w in oracle.items()}

    def launch(T, ws):
        op.run({k: v for k, v in T.items() if v is not None}, ws)
    got = guard_launch(family, op.name, arrays, outs, launch, op.ws_bytes, "%s %s" % (op.name, what))
    op.check(got, oracle)
    for n in oracle:
        if n not in op.prev:
            GU.assert_no_sentinel_run(got[n], "%s %s, output '%s'" % (op.name, what, n))


@pytest.mark.parametrize("seed", range(6))
def test_pooling_eltwise_fc_random_shapes(seed):
    """the cases of test_pooling_eltwise_fc_random_shapes_vs_oracle (its generator, seeds 0..5), every tensor guarded"""
    names = []
    for i, (op, arrays, oracle) in enumerate(TP.gen_pooling_eltwise_fc(seed)):
        _guard_stream("stream", op, arrays, oracle, "seed %d case %d %s" % (seed, i, {n: a.shape for n, a in arrays.items()}))
        names.append(op.name)
    print("seed %d: %s" % (seed, " ".join(names)))


@pytest.mark.parametrize("seed", range(4))
def test_layout_quant_softmax_gemm_random_shapes(seed):
    """the cases of test_layout_quant_softmax_gemm_random_shapes_vs_oracle (its generator, seeds 0..3), every tensor guarded"""
    names = []
    for i, (op, arrays, oracle) in enumerate(TP.gen_layout_quant_softmax_gemm(seed)):
        _guard_stream("stream", op, arrays, oracle, "seed %d case %d %s" % (seed, i, {n: a.shape for n, a in arrays.items()}))
        names.append(op.name)
    print("seed %d: %s" % (seed, " ".join(names)))


def _eq(what):
    def check(got, want):
        for n, w in want.items():
            assert got[n].shape == w.shape and np.array_equal(got[n], w), (what, n)
    return check


@pytest.mark.parametrize("n", [1, 15, 17, 4099])
def test_flat_ops_at_counts_beside_the_vector_width(n):
    """eltwise sum (s8, f32), relu, an activation, prelu and the flat quantisation on n elements: one vector is 16 bytes / 4 floats"""
    rng = np.random.default_rng(5700 + n)
    a, b = rng.integers(-128, 128, n).astype(np.int8), rng.integers(-128, 128, n).astype(np.int8)
    fa, fb = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    k8, kf = ((1.7, 2.9), True, 0.05, 0.043), ((1.7, 2.9), True)
    _guard_stream("stream", TP.StreamOp("eltwise_sum_i8", lambda T, ws=None: {"y": S.eltwise_sum(T["a"], T["b"], *k8, out=T["y"])}, _eq("eltwise i8")),
                  {"a": a, "b": b}, {"y": O.eltwise_i8(a, b, 0.05, 0.043, 1.7, 2.9, True)}, "n=%d" % n)
    _guard_stream("stream", TP.StreamOp("eltwise_sum_f32", lambda T, ws=None: {"y": S.eltwise_sum(T["a"], T["b"], *kf, out=T["y"])}, _eq("eltwise f32")),
                  {"a": fa, "b": fb}, {"y": O.eltwise_f32(fa, fb, 1.7, 2.9, True)}, "n=%d" % n)
    x = (fa * 3).astype(np.float32)
    for active, slope, coef in ((S.ACTIVE_RELU, 0.0, 1.0), (S.ACTIVE_RELU, 0.3, 1.0), (S.ACTIVE_SIGMOID, 0.0, 1.0)):
        want = O.activation_f32(x, active, slope, coef)

        def check(got, w, active=active):          # test_activation_types_vs_oracle's criterion
            assert np.abs(got["y"] - w["y"]).max() <= FP32_RTOL * max(np.abs(w["y"]).max(), 1e-3), active
        _guard_stream("stream", TP.StreamOp("activation_%d" % active, lambda T, ws=None, k=(active, slope, coef): {"y": S.activation(k[0], T["x"], T["y"], k[1], k[2])},
                                            check), {"x": x}, {"y": want}, "n=%d" % n)
    slope = (rng.standard_normal(n) * 0.5).astype(np.float32)
    _guard_stream("stream", TP.StreamOp("prelu", lambda T, ws=None: {"y": S.prelu(T["x"], T["slope"], n, 1, False, T["y"])}, _eq("prelu")),
                  {"x": x, "slope": slope}, {"y": O.prelu_f32(x.reshape(1, n), slope, 1, False).reshape(n)}, "n=%d" % n)
    flat = (fa * 30).astype(np.float32)
    _guard_stream("stream", TP.StreamOp("quantize_flat_s8", lambda T, ws=None: {"y": S.quantize_flat_s8(T["x"], 0.37, out=T["y"])}, _eq("flat quantise")),
                  {"x": flat}, {"y": O.quant_flat_s8(flat, 0.37)}, "n=%d" % n)


@pytest.mark.parametrize("shape", [(2, 3, 5, 7, 4), (1, 5, 3, 3, 8), (1, 17, 4, 5, 20)])
def test_quantise_and_transpose_with_channel_padding(shape):
    """c_pad > c: the pad lanes of every pixel are written as zeros, nothing past the last pixel"""
    n, c, h, w, c_pad = shape
    rng = np.random.default_rng(5800 + c)
    x = (rng.standard_normal((n, c, h, w)) * 40.0).astype(np.float32)
    for odt in (S8, U8):
        want = np.zeros((n, h, w, c_pad), NP_DT[odt])
        want[..., :c] = O.quant_nchw_to_nhwc(x, 0.37, odt)
        _guard_stream("stream", TP.StreamOp("quantize_nchw_to_nhwc", lambda T, ws=None, o=odt: {"y": S.quantize_nchw_to_nhwc(T["x"], 0.37, o, c_pad, out=T["y"])},
                                            _eq("quantise c_pad")), {"x": x}, {"y": want}, str(shape))
    t_ref = np.zeros((n, h, w, c_pad), np.float32)
    t_ref[..., :c] = x.transpose(0, 2, 3, 1)
    _guard_stream("stream", TP.StreamOp("transpose_nchw_to_nhwc", lambda T, ws=None: {"y": S.transpose_nchw_to_nhwc(T["x"], c_pad, out=T["y"])}, _eq("transpose in")),
                  {"x": x}, {"y": t_ref}, str(shape))
    _guard_stream("stream", TP.StreamOp("transpose_nhwc_to_nchw", lambda T, ws=None: {"y": S.transpose_nhwc_to_nchw(T["x"], c, out=T["y"])}, _eq("transpose out")),
                  {"x": t_ref}, {"y": x}, str(shape))


def test_pooling_edges():
    """max pooling at C = 16 (the 16-byte vector path) and C = 24, the global average at (1, 5, 9, 132), pooling_f32_from_i8 with and without
    the fused quantisation of its result"""
    rng = np.random.default_rng(5900)
    for C in (16, 24):
        for dt in (S8, U8):
            x = _rand8(rng, (2, 9, 7, C), dt)
            _guard_stream("stream", TP.StreamOp("pooling_i8_max_c%d" % C, lambda T, ws=None: {"y": S.pooling_i8(T["x"], (3, 3), (2, 2), (1, 1), 0, out=T["y"])},
                                                _eq("max pool")), {"x": x}, {"y": O.pool_i8_nhwc(x, (3, 3), (2, 2), (1, 1), 0)}, "C=%d" % C)
    for dt in (S8, U8):
        x = _rand8(rng, (1, 5, 9, 132), dt)
        _guard_stream("stream", TP.StreamOp("pooling_i8_global_avg", lambda T, ws=None: {"y": S.pooling_i8(T["x"], None, None, None, 1, global_pooling=True, out=T["y"])},
                                            _eq("global average")), {"x": x}, {"y": O.pool_i8_nhwc(x, None, None, None, 1, global_pool=True)}, "(1, 5, 9, 132)")
        x = _rand8(rng, (2, 13, 13, 24), dt)
        want = O.pool_f32_nchw(O.dequant_nhwc_to_nchw(x, 0.05), (3, 3), (2, 2), (1, 1), 0)
        _guard_stream("stream", TP.StreamOp("pooling_f32_from_i8", lambda T, ws=None: {"y": S.pooling_f32_from_i8(T["x"], 0.05, (3, 3), (2, 2), (1, 1), 0, out=T["y"])},
                                            _eq("pool f32 from i8")), {"x": x}, {"y": want}, "3x3 / 2")

        def run_q(T, ws=None):
            y, yq = S.pooling_f32_from_i8(T["x"], 0.05, (3, 3), (2, 2), (1, 1), 0, q_scale=0.011, out=T["y"], out_q=T["yq"])
            return {"y": y, "yq": yq}
        _guard_stream("stream", TP.StreamOp("pooling_f32_from_i8_q", run_q, _eq("pool f32 from i8 + q")), {"x": x},
                      {"y": want, "yq": O.quant_flat_s8(want, 0.011)}, "3x3 / 2")
        x = _rand8(rng, (3, 7, 7, 200), dt)
        want = O.pool_f32_nchw(O.dequant_nhwc_to_nchw(x, 0.37), None, None, None, 1, global_pool=True)

        def run_gq(T, ws=None):
            y, yq = S.pooling_f32_from_i8(T["x"], 0.37, None, None, None, 1, global_pooling=True, q_scale=0.2, out=T["y"], out_q=T["yq"])
            return {"y": y, "yq": yq}
        _guard_stream("stream", TP.StreamOp("pooling_f32_from_i8_global_q", run_gq, _eq("global pool f32 from i8 + q")), {"x": x},
                      {"y": want, "yq": O.quant_flat_s8(want, 0.2)}, "global")


@pytest.mark.parametrize("shape", [(3, 1001), (1, 1)])
def test_softmax_edges(shape):
    z = (np.random.default_rng(6000 + shape[1]).standard_normal(shape) * 10.0).astype(np.float32)

    def check(got, w):          # test_layout_quant_softmax_gemm_random_shapes_vs_oracle's criterion
        assert np.abs(got["y"] - w["y"]).max() <= FP32_RTOL * w["y"].max() and np.allclose(got["y"].sum(1), 1.0, atol=1e-5)
    _guard_stream("stream", TP.StreamOp("softmax", lambda T, ws=None: {"y": S.softmax(T["x"], out=T["y"])}, check), {"x": z}, {"y": O.softmax_f32(z)}, str(shape))


def _fc_softmax_run(fc):
    def run(T, ws=None):
        if ws is not None:
            fc.ws = ws
        fc.dispatch_softmax(T["x"], T["y"], T["prob"])
        return {"y": T["y"], "prob": T["prob"]}
    return run


@pytest.mark.parametrize("shape", [(1, 1000, 2048), (5, 24, 4096), (3, 1000, 528)])
@pytest.mark.parametrize("idt", [S8, U8])
def test_fc_i8_small_batch(shape, idt):
    """test_fc_small_batch_kernel's recipe: the small-batch kernel and the implicit-GEMM form behind the same op"""
    M, N, K = shape
    rng = np.random.default_rng(6100 + M + N + idt)
    wq = rng.integers(-127, 128, (N, K)).astype(np.int8)
    ws = (rng.random(N).astype(np.float32) * 0.01 + 0.001)
    b = rng.standard_normal(N).astype(np.float32)
    x = _rand8(rng, (M, K), idt)
    fc = S.SaberFc(True).init(M, N, K, wq, b, idt, 0.031, 0.5, w_scale=ws)
    assert fc.algo() == "fc_i8_small_16xk4", fc.algo()
    want = O.fc_i8(x, wq, ws, 0.031, b, 0.5) if idt == U8 else O.fc_i8(x, wq, ws, 0.031, b)
    _guard_stream("fc", TP.StreamOp(fc.algo(), TP._fc_run(fc), _eq("fc i8"), TP._fc_ws(fc)), {"x": x}, {"y": want}, str(shape))
    fc.set_tile(0 | (4 << 8) | (1 << 16))
    assert fc.algo().startswith("igemm_i8"), fc.algo()
    _guard_stream("fc", TP.StreamOp("fc:" + fc.algo(), TP._fc_run(fc), _eq("fc i8"), TP._fc_ws(fc)), {"x": x}, {"y": want}, str(shape))


@pytest.mark.parametrize("shape", [(2, 512, 10), (8, 1024, 333)])
def test_fc_i8_softmax_in_one_launch(shape):
    M, K, N = shape
    rng = np.random.default_rng(300 + M + K + N)
    w = (rng.standard_normal((N, K)) * 0.02).astype(np.float32)
    b = rng.standard_normal(N).astype(np.float32)
    ws = O.weight_scales(w)
    wq = O.quant_weights(w, ws)
    for dt in (S8, U8):
        fc = S.SaberFc(True).init(M, N, K, wq, b, dt, 0.031, 0.5 if dt == U8 else 1.0, w_scale=ws)
        x = _rand8(rng, (M, K), dt)
        want = O.fc_i8(x, wq, ws, 0.031, b, 0.5) if dt == U8 else O.fc_i8(x, wq, ws, 0.031, b)

        def check(got, w_):          # test_fc_i8_softmax_in_one_launch's criteria
            assert np.array_equal(got["y"], w_["y"])
            assert np.abs(got["prob"] - w_["prob"]).max() <= FP32_RTOL * w_["prob"].max() and np.allclose(got["prob"].sum(1), 1.0, atol=1e-5)
        _guard_stream("fc", TP.StreamOp(fc.algo() + "+softmax", _fc_softmax_run(fc), check, TP._fc_ws(fc)), {"x": x},
                      {"y": want, "prob": O.softmax_f32(want)}, str(shape))


@pytest.mark.parametrize("shape", [(3, 512, 40), (5, 2048, 1001)])
def test_fc_f32_split_k(shape):
    """fc_f32_splitk.hip (opt-in through the environment, read by set_weights) and its fused softmax (<= 1024 outputs)"""
    import os
    M, K, N = shape
    rng = np.random.default_rng(77 + M + K + N)
    w = (rng.standard_normal((N, K)) * np.sqrt(1.0 / K)).astype(np.float32)
    b = rng.standard_normal(N).astype(np.float32)
    x = rng.standard_normal((M, K)).astype(np.float32)
    os.environ["SABER_HIP_FC_F32_SPLITK"] = "1"
    try:
        fc = S.SaberFc(False).init(M, N, K, w, b, L.F32)
    finally:
        del os.environ["SABER_HIP_FC_F32_SPLITK"]
    assert fc.algo() == "fc_f32_splitk_16xk4", fc.algo()
    want = O.fc_f32(x, w, b)

    def check(got, w_):              # test_fc_f32_split_k_and_softmax_in_one_launch's criteria
        assert_f32(got["y"], w_["y"], "fc f32 split-K %s" % (shape,))
        if "prob" in w_:
            assert np.abs(got["prob"] - w_["prob"]).max() <= FP32_RTOL * w_["prob"].max()
    _guard_stream("fc", TP.StreamOp(fc.algo(), TP._fc_run(fc), check, TP._fc_ws(fc)), {"x": x}, {"y": want}, str(shape))
    if N <= 1024:
        _guard_stream("fc", TP.StreamOp(fc.algo() + "+softmax", _fc_softmax_run(fc), check, TP._fc_ws(fc)), {"x": x},
                      {"y": want, "prob": O.softmax_f32(want)}, str(shape))


@pytest.mark.parametrize("ta,tb", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_gemm_f32(ta, tb):
    """Gemm f32 with beta = 1 into a guarded C: (37, 50, 72) and (16, 515, 4104) take the bf16-plane path (k % 8 == 0 is its condition,
    test_gemm_f32_plane_path_vs_oracle), (37, 50, 45) the f32-MFMA kernel"""
    rng = np.random.default_rng(6200 + 2 * ta + tb)
    for (M, N, K), name in (((37, 50, 72), "gemm_f32_plane_k72"), ((16, 515, 4104), "gemm_f32_plane_k4104"), ((37, 50, 45), "gemm_f32_mfma_k45")):
        A = rng.standard_normal((K, M) if ta else (M, K)).astype(np.float32)
        B = rng.standard_normal((N, K) if tb else (K, N)).astype(np.float32)
        C0 = rng.standard_normal((M, N)).astype(np.float32)
        a64, b64 = (A.T if ta else A).astype(np.float64), (B.T if tb else B).astype(np.float64)
        want = (a64 @ b64 + C0).astype(np.float32)

        def check(got, w_, what=(name, ta, tb)):     # test_gemm_f32_plane_path_vs_oracle's two measures
            assert_f32(got["c"], w_["c"], "%s ta=%d tb=%d" % what)
        _guard_stream("gemm", TP.StreamOp("%s_t%d%d" % (name, ta, tb), lambda T, ws=None, k=(ta, tb, M, N, K): {"c": S.gemm(*k, 1.0, T["a"], T["b"], 1.0, T["c"])},
                                          check, prev={"c": C0}), {"a": A, "b": B}, {"c": want}, str((M, N, K)))


@pytest.mark.parametrize("ta,tb", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("adt", [S8, U8])
def test_gemm_i8(ta, tb, adt):
    """test_gemm_i8_exact's shapes: int32 results equal the integer matrix product, A, C and the workspace guarded"""
    rng = np.random.default_rng(6300 + 4 * adt + 2 * ta + tb)
    for M, N, K in ((70, 130, 45), (8, 1000, 2048), (33, 64, 4000)):
        A = _rand8(rng, (M, K), adt)
        B = rng.integers(-128, 128, (K, N)).astype(np.int8)
        if (M, N, K) == (33, 64, 4000):
            A[:] = 255 if adt == U8 else -128
            B[:, ::2] = -128
            B[:, 1::2] = 127
        want = (A.astype(np.int64) @ B.astype(np.int64)).astype(np.int32)
        g = S.GemmInt8().init(ta, tb, M, N, K, np.ascontiguousarray(B.T) if tb else B, adt)

        def run(T, ws=None, g=g):
            if ws is not None:
                g.ws = ws
            return {"c": g.dispatch(T["a"], T["c"])}
        wsb = int(L.load().saber_hip_gemm_i8_workspace_bytes(g.h))
        _guard_stream("gemm", TP.StreamOp("gemm_i8_%s_t%d%d" % (P.DT_NAME[adt], ta, tb), run, _eq("gemm i8"), wsb),
                      {"a": np.ascontiguousarray(A.T) if ta else A}, {"c": want}, str((M, N, K)))


# ==== net level =============================================================================================================================
from anakin_amd import workloads as W  # noqa: E402

_NET_INPUTS = {}


def _net_inputs(name, batch, hw):
    """(framework model, scales, input) - computed once and never changed; the oracle is not needed here (the unbound net is pinned to it by
    tests/test_gpu_stage_tail.py / tests/test_gpu_sep.py)"""
    if (name, batch, hw) not in _NET_INPUTS:
        model = W.build_model(name)
        fw = W.framework_model(model, "int8")
        x = W.make_input(batch, hw=hw)
        # (the routes of tests/test_gpu_stage_tail.py and tests/test_gpu_sep.py: ResNet50 is calibrated on its framework list)
        _NET_INPUTS[(name, batch, hw)] = (fw, W.calibrate(fw if name == "resnet50" else model, x[:2]), x)
    return _NET_INPUTS[(name, batch, hw)]


def _bind_every_tensor(pattern, store):
    """build_int8_net's before_finalize callback: EVERY tensor of the net (the ones the optimiser leaves unwritten too) lives in a guarded
    buffer of exactly its byte count, aligned to 16 bytes and no more, pre-filled with the sentinel"""
    def bind(net):
        lib = L.load()
        for tid in range(net.num_tensors()):
            g = GU.Guarded((int(lib.saber_hip_net_tensor_bytes(net.h, tid)),), torch.uint8, pattern, "cuda")
            store[tid] = g
            net.keep.append(g)
            L.check(lib.saber_hip_net_bind_tensor(net.h, tid, g.ptr))      # (Net.bind by address: an empty tensor has no data_ptr)
    return bind


def _written_edges(net):
    torch.cuda.synchronize()
    return {nm: net.tensor(nm).cpu().numpy() for nm in net.tensors if nm != "data" and not net.unwritten(nm)}


def _net_passes(net, x, what, guards=None):
    """eager pass, then capture + replay; returns the written edges after each and checks the guards after each"""
    out = {}
    for form in ("eager", "replayed"):
        for nm in net.tensors:
            if nm != "data" and not net.unwritten(nm):
                net.tensor(nm).fill_(GU.SENTINEL) if net.tensor(nm).dtype != torch.float32 else net.tensor(nm).fill_(-7.0)
        net.tensor("data").copy_(torch.from_numpy(x).cuda())
        if form == "eager":
            net.run()
        else:
            net.capture()
            net.replay()
        out[form] = _written_edges(net)
        net.status()
        if guards is not None:
            names = {tid: nm for nm, (tid, _, _) in net.tensors.items()}
            GU.assert_footprint({"%s (tensor %d)" % (names.get(tid, "-"), tid): g for tid, g in guards.items()}, "%s, %s pass" % (what, form))
    return out


@pytest.mark.parametrize("which", ["resnet50", "mobilenet_v1"])
def test_net_with_every_tensor_in_a_guarded_buffer(which):
    """ResNet50 INT8 (framework list, batch 3, 96 x 96, stages and tails selected) and MobileNet-v1 INT8 (separable sites on, batch 1,
    96 x 96), built as always and built with every tensor bound to a guarded buffer before finalize: the same choices, op names and launch
    count (so the same fused forms run), every written edge byte-identical, eager and replayed, every guard intact after each pass, for both
    patterns. Inside the arena a stray store lands in slot slack or in a neighbouring edge; here it lands in a guard.
    Limit: only the edge tensors are guarded and pre-filled here. The net's own workspace belongs to the library (zeroed once when the
    arena is made) and is neither guarded nor dirtied at this level; the per-op tests above hand every op a dirty guarded workspace."""
    batch = 3 if which == "resnet50" else 1
    fw, scales, x = _net_inputs(which, batch, 96)

    def build(cb=None):
        if which == "resnet50":
            net = W.build_int8_net(fw, dict(scales), batch, hw=96, stage=True, before_finalize=cb)
            net.select_stages(True)
            net.select_tails(True)
        else:
            net = W.build_int8_net(fw, dict(scales), batch, hw=96, separable=True, before_finalize=cb)
            TS.force_on(net)
        return net
    plain = build()
    names = [plain.op_name(i) for i in range(plain.num_ops())]
    if which == "resnet50":
        assert plain.tails() and all(s[2] for s in plain.stages()), (plain.stages(), plain.tails())
    else:
        assert plain.separated == 13 and sum("sep_dw3x3_pw_i8_" in n for n in names) == 13, names
    ref = _net_passes(plain, x, which + ", arena")
    assert len(ref["eager"]) >= 15 and all(GU.same_bytes(ref["eager"][n], ref["replayed"][n]) for n in ref["eager"])
    print("%s: %d ops in %d launches: %s" % (which, plain.num_ops(), plain.num_launches(), " ".join(sorted(set(names)))))
    REACHED.setdefault("net", set()).update(names)
    for pat in GU.PATTERNS:
        store = {}
        net = build(_bind_every_tensor(pat, store))
        assert len(store) == net.num_tensors() >= len(net.tensors)
        assert net.choices() == plain.choices() and net.num_launches() == plain.num_launches()
        assert [net.op_name(i) for i in range(net.num_ops())] == names
        got = _net_passes(net, x, "%s, %s" % (which, GU.label(pat)), store)
        for form in ("eager", "replayed"):
            assert sorted(got[form]) == sorted(ref[form]), (form, sorted(set(got[form]) ^ set(ref[form])))
            for nm, a in ref[form].items():
                assert GU.same_bytes(got[form][nm], a), "%s, %s, %s pass: edge '%s' differs from the arena net's" % (which, GU.label(pat), form, nm)


# ==== the harness on the device, and the coverage of the file ===============================================================================
def test_guards_on_the_device_report_the_first_changed_byte():
    """guard_util on device memory: torch writes one byte before, one byte after and far into the back guard of a guarded tensor"""
    g = GU.guarded((3, 5), np.float32, 0xFF, "cuda")
    assert g.t.is_cuda and g.t.data_ptr() % 256 == 16 and g.intact() is None
    g.buf[g.hi] = 0
    assert g.intact() == (None, 0)
    g.buf[g.hi] = 0xFF
    g.buf[g.lo - 1] = 1
    g.buf[g.hi + 70000] = 2
    assert g.intact() == (-1, 70000)
    with pytest.raises(AssertionError, match="tensor 'y'.*front guard, first changed byte 1 before"):
        GU.assert_footprint({"y": g}, "device")


def _family_key(name):
    """a kernel name without its tile and its numbers: igemm_i8_64x32_k2_dma -> igemm_i#_, halo3x3_f32_bf16x3_64ch_4x16_w4 -> halo#x#_f#_bf#x#_#ch_"""
    import re
    m = re.sub(r"\d+", "#", name.split("+")[0])
    m = re.sub(r"^(halo|img|imgres|stem|pw|dw|g)#x#", r"\1", m)
    return m.split("#x#")[0]


def test_guarded_launches_reached_every_form_family():
    """Asserts on the names guard_launch recorded while the tests above RAN in this session (run the whole file: alone, this test fails).
    Two checks. The families the issue lists, by name. And, so that a new family is noticed without anybody editing this file: every kernel
    family the probe suites' own geometry lists enumerate (P.GEOMETRIES with TI._forms, FP.CONV_GEOMETRIES with TF._forms - the lists a new
    kernel is added to for its probes) must have had a guarded launch here."""
    missing = [f for f in ("conv_i8", "conv_f32", "imgres", "stem_pool_i8", "conv_f32_pool", "stem_f32", "pair_i8", "pair_f32", "chain1x1", "chain3x3",
                           "head", "stem_pair", "stage", "tail", "xcd_stage", "sep", "dw", "group", "fc", "gemm", "stream", "net") if f not in REACHED]
    assert not missing, "no guarded launch ran for %s (run the whole file)" % missing
    reached = {k: set(v) for k, v in REACHED.items()}
    enumerated = set()
    for gn in P.GEOMETRIES:
        if not gn.startswith("stempool"):
            enumerated |= {a for _, a in TI._forms(TI.make_conv(P.build("conv/%s/u8u8/relu1" % gn)))}
    rng = np.random.default_rng(3)
    for gn, geo in FP.CONV_GEOMETRIES.items():
        N, H, W, C, K, k, pad, stride, dil = geo
        w = rng.standard_normal((K, C, k, k)).astype(np.float32)
        enumerated |= {a for _, a in TF._forms(TF._make_conv(geo, w, None, layout=L.NCHW if gn.endswith("_nchw") else L.NHWC))}
    ran = {_family_key(a) for fam in ("conv_i8", "conv_f32", "imgres") for a in reached[fam]}
    unguarded = sorted({_family_key(a) for a in enumerated} - ran)
    print("kernel families of the probe geometries: %s" % sorted({_family_key(a) for a in enumerated}))
    assert not unguarded, "kernel families the probe suites enumerate that no guarded launch ran: %s" % unguarded
    i8, f32 = reached["conv_i8"], reached["conv_f32"]
    pw = [a for a in f32 if a.startswith("pw1x1_f32_bf16x3_")]
    want = {
        # the families of test_conv_i8_probe_geometries_reach_every_form_family
        "INT8 implicit GEMM": [a for a in i8 if a.startswith("igemm_i8")], "INT8 halo 3x3": [a for a in i8 if a.startswith("halo3x3_i8")],
        "INT8 image-resident 3x3": [a for a in i8 if a.startswith("img3x3_i8")], "INT8 stem": [a for a in i8 if a.startswith("stem7x7s2_i8")],
        "INT8 image-resident 1x1": [a for a in i8 | reached["imgres"] if a.startswith("imgres1x1_i8")],
        "INT8 image-resident 3x3 (whole image)": [a for a in i8 | reached["imgres"] if a.startswith("imgres3x3_i8")],
        "INT8 stem + max pooling": reached["stem_pool_i8"], "fused global pooling": [a for a in reached["imgres"] if a.endswith("+gpool")],
        # FP32
        "FP32 bf16-plane implicit GEMM": [a for a in f32 if a.startswith("igemm_f32_bf16x3") and "_split" not in a],
        "FP32 bf16-plane split-K": [a for a in f32 if a.startswith("igemm_f32_bf16x3") and "_split" in a],
        "FP32 8-wave tile": [a for a in f32 if a.startswith("igemm_f32_bf16x3") and "_w8" in a],
        "FP32 f32 MFMA": [a for a in f32 if a.startswith("igemm_f32_") and "bf16x3" not in a],
        "FP32 halo 3x3": [a for a in f32 if a.startswith("halo3x3_f32_bf16x3")],
        "FP32 pointwise": [a for a in pw if "_regs_" not in a and "_ksplit4_" not in a],
        "FP32 register-weights pointwise": [a for a in pw if "_regs_" in a], "FP32 reduction-split pointwise (pwk)": [a for a in pw if "_ksplit4_" in a],
        "FP32 conv + max pooling": reached["conv_f32_pool"], "FP32 stem": reached["stem_f32"],
        # multi-tensor launches
        "INT8 pair": [a for a in reached["pair_i8"] if a.startswith("pair_igemm_i8")], "FP32 pair": [a for a in reached["pair_f32"] if a.startswith("pair_igemm_f32")],
        "1x1 chain": reached["chain1x1"], "3x3-led chain": reached["chain3x3"], "strided head": [a for a in reached["head"] if a.startswith("head_c")],
        "strided head + pair": [a for a in reached["head"] if a.startswith("head_pair")], "stem pair": reached["stem_pair"],
        "chain stage": reached["stage"], "stage tail": reached["tail"], "XCD stage": reached["xcd_stage"],
        "separable": [a for a in reached["sep"] if a.startswith("sep_dw3x3_pw_i8_")],
        "depthwise INT8": [a for a in reached["dw"] if a.startswith("dw3x3_i8_")], "depthwise FP32": [a for a in reached["dw"] if a.startswith("dw3x3_f32_")],
        "grouped 3x3": [a for a in reached["group"] if a.startswith("g3x3_i8_")],
        "direct": [a for a in reached["dw"] | reached["group"] if a.startswith("direct_")],
        # streaming, fc, GEMM
        "fc": reached["fc"], "GEMM": reached["gemm"], "streaming": reached["stream"],
    }
    print({k: len(v) for k, v in want.items()})
    for fam, names in sorted(reached.items()):
        if fam != "net":
            print("%s (%d): %s" % (fam, len(names), " ".join(sorted(names))))
    assert all(want.values()), sorted(k for k, v in want.items() if not v)
    # the 3x3-led chain runs its cooperative forms where the device places them, and both chain kinds more than one form
    assert {"stage_c256", "stage_c128", "stage_c64", "stage_c64_inner_y1_null"} <= reached["stage"], sorted(reached["stage"])
    assert len(reached["chain1x1"]) >= 8 and len(reached["chain3x3"]) >= 12, (sorted(reached["chain1x1"]), sorted(reached["chain3x3"]))
    stream = {"pooling_i8", "pooling_f32_nchw", "pooling_f32_nhwc", "eltwise_sum_i8", "eltwise_sum_f32", "quantize_nchw_to_nhwc",
              "dequantize_nhwc_to_nchw", "transpose_nchw_to_nhwc", "transpose_nhwc_to_nchw", "quantize_flat_s8", "softmax", "gemm_f32"}
    assert stream <= reached["stream"], sorted(stream - reached["stream"])
