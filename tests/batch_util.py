"""Batch sizes beyond 8 and streaming launches beyond one grid stride: the case tables and references that tests/test_batch_cpu.py checks
and tests/test_gpu_batch.py runs. TEST INFRASTRUCTURE ONLY; nothing here needs a GPU.

Part A: every launch form at N = 9 (the first batch beyond the XCD count and the stage limit), N = 17 (odd, the first beyond the
small-batch fc kernels) and, for the single convolutions, N = 33 (odd, beyond the published batch 32), at each family's smallest
spatial sizes. Expected values are the oracle's, computed once per (case, N) and never modified; every image of a case is a different
seeded random image, so no two images' expected outputs are equal and an image index taken modulo 8, 16 or 32 changes bytes.

Part B: one case per streaming launcher of anakin_amd/csrc/elementwise.hip whose work-item count lies between one and two grid
strides, by a ragged amount; the references are plain numpy, pinned to the oracle on a slice by the CPU test."""
import numpy as np

from oracle import oracle as O

F32, S8, U8 = O.F32, O.S8, O.U8
NP_DT = {F32: np.float32, S8: np.int8, U8: np.uint8}

# anakin_amd/csrc/elementwise.hip: grid_for() caps a streaming launch at 8 192 blocks, and launch_quantize_nchw_to_nhwc (both kernels) and
# launch_dequantize_nhwc_to_nchw spell the same cap inline; every block has 256 lanes. A launch with more work items than this takes
# its lanes round the grid-stride loop a second time.
GRID_CAP_BLOCKS = 8192
BLOCK_LANES = 256
GRID_CAP = GRID_CAP_BLOCKS * BLOCK_LANES      # 2 097 152

BATCHES = (9, 17, 33)
BATCHES_COMPOSITE = (9, 17)
XCDS, STAGE_MAX_BATCH, FC_SMALL_MAX_ROWS, PUBLISHED_BATCH, GRID_Y_MAX = 8, 8, 16, 32, 65535


def rand8(rng, shape, dt):
    return (rng.integers(0, 256, shape) if dt == U8 else rng.integers(-128, 128, shape)).astype(NP_DT[dt])


def distinct_images(y):
    """no two images of the batch-major array y are equal"""
    return len({np.ascontiguousarray(y[i]).tobytes() for i in range(y.shape[0])}) == y.shape[0]


# ---- part A: single INT8 convolutions ------------------------------------------------------------------------------------------------------
# h, w, c, k, kernel, pad, stride, group, input (F32: an f32 NCHW image quantised on entry), output, relu, residual kind
#   residual: None | "elt" fused eltwise with the unequal coefficients (c, -c / 2) | "sum" in-place sum onto the bytes in the output |
#             "sub" fused eltwise whose shortcut is read sub-sampled (res_stride = 2)
I8_CONVS = {
    "pw_64_256":    (7, 9, 64, 256, 1, 0, 1, 1, U8, U8, 1, None),
    "c3x3_64":      (7, 9, 64, 64, 3, 1, 1, 1, U8, U8, 1, None),        # implicit GEMM, LDS halo, small-image kernel (1 and 2 images per slab)
    "c3x3_64_s2":   (7, 9, 64, 64, 3, 1, 2, 1, S8, S8, 0, None),
    "pw_64_128_s2": (5, 17, 64, 128, 1, 0, 2, 1, U8, S8, 0, None),
    "stem_f32":     (30, 30, 3, 64, 7, 3, 2, 1, F32, U8, 1, None),
    "stem_s8":      (30, 30, 3, 64, 7, 3, 2, 1, S8, S8, 0, None),
    "dw_32_s1":     (7, 9, 32, 32, 3, 1, 1, 32, U8, U8, 1, None),
    "dw_32_s2":     (5, 17, 32, 32, 3, 1, 2, 32, S8, S8, 0, None),
    "g16_64":       (7, 9, 64, 64, 3, 1, 1, 16, U8, U8, 1, None),
    "g2_64":        (7, 9, 64, 64, 3, 1, 1, 2, S8, S8, 0, None),
    "c3_5x5":       (7, 9, 3, 8, 5, 2, 1, 1, U8, S8, 0, None),          # C = 3 is padded to 4: the NHWC4 implicit GEMM (igemm_i8_c4), not the direct kernel
    "direct_g2_5x5": (7, 9, 6, 8, 5, 2, 1, 2, U8, S8, 0, None),         # three channels per group, 5 x 5: only the direct kernel takes it
    "pw_elt_pair":  (7, 9, 64, 256, 1, 0, 1, 1, U8, S8, 0, "elt"),
    "c3x3_32_sum":  (7, 7, 32, 32, 3, 1, 1, 1, S8, U8, 1, "sum"),
    "pw_sub_res":   (7, 7, 64, 128, 1, 0, 1, 1, U8, S8, 0, "sub"),
}
I8_IN_SCALE, I8_OUT_SCALE, I8_RES_SCALE, I8_SUM_SCALE, I8_ELT_OUT_SCALE = 0.02, 0.05, 0.043, 0.37, 0.06
I8_ELT_PAIR = (1.0, -0.5)

_cache = {}


class I8Conv:
    """One (case, N): operands, parameters and the oracle's bytes. x is what the device op reads (f32 NCHW for an F32 input, else
    8-bit NHWC); res / prev the fused eltwise's second operand / the bytes the in-place sum starts from."""

    def __init__(self, name, n):
        h, w, c, k, ks, pad, stride, group, idt, odt, relu, kind = I8_CONVS[name]
        self.name, self.n, self.geo, self.kind = name, n, I8_CONVS[name], kind
        rng = np.random.default_rng([20280, sorted(I8_CONVS).index(name), n])
        self.in_scale, self.out_scale = (1.0 / 127 if idt == F32 else I8_IN_SCALE), I8_OUT_SCALE
        if idt == F32:
            self.x = rng.uniform(-1, 1, (n, c, h, w)).astype(np.float32)
            xq, qdt = O.quant_nchw_to_nhwc(self.x, self.in_scale, S8), S8
        else:
            self.x = rand8(rng, (n, h, w, c), idt)
            xq, qdt = self.x, idt
        self.w = (rng.standard_normal((k, c // group, ks, ks)) * np.sqrt(2.0 / (c // group * ks * ks))).astype(np.float32)
        self.b = (rng.standard_normal(k) * 0.5).astype(np.float32)
        ws = O.weight_scales(self.w)
        wq = O.quant_weights(self.w, ws)
        bp, sc = O.conv_i8_prepare(ws, self.b, self.in_scale, self.out_scale, qdt, odt)
        geo = ((pad, pad), (stride, stride), (1, 1), group)
        self.res = self.res_hw = self.prev = self.coeff = None
        if kind == "sum":
            y = O.conv_i8(xq, wq, bp, sc, odt, relu, *geo)
            self.prev = rand8(rng, y.shape, odt)
            rp = O.Residual(O.RES_JIT_SUM, 0, I8_SUM_SCALE, odt, 0, 0, 0, 0)
            self.want = O.conv_i8(xq, wq, bp, sc, odt, relu, *geo, residual=rp, out_init=self.prev)
        elif kind in ("elt", "sub"):
            y = O.conv_i8(xq, wq, bp, sc, S8, 0, *geo)
            cf = 1.0 / I8_ELT_OUT_SCALE
            self.coeff = (float(np.float32(I8_ELT_PAIR[0] * cf)), float(np.float32(I8_ELT_PAIR[1] * cf))) if kind == "elt" else (cf, cf)
            if kind == "sub":
                oh, ow = y.shape[1:3]
                self.res_hw = (2 * oh - 1, 2 * ow - 1)      # (hs - 1) // 2 + 1 == oh: a ragged shortcut
                self.res = rand8(rng, (n,) + self.res_hw + (k,), S8)
                r = O.pool_i8_nhwc(self.res, (1, 1), (2, 2), (0, 0), 0, floor_mode=True)
                assert r.shape == y.shape
            else:
                self.res = r = rand8(rng, y.shape, S8)
            self.want = O.eltwise_i8(y, r, self.out_scale, I8_RES_SCALE, self.coeff[0], self.coeff[1], True)
        else:
            self.want = O.conv_i8(xq, wq, bp, sc, odt, relu, *geo)


def i8_conv(name, n):
    if (name, n) not in _cache:
        _cache[name, n] = I8Conv(name, n)
    return _cache[name, n]


# ---- part A: FP32 convolutions (NHWC on the device, NCHW here) ----------------------------------------------------------------------------------
# h, w, c, k, kernel, pad, group
F32_CONVS = {
    "c3x3_64":   (7, 9, 64, 64, 3, 1, 1),
    "pw_256_64": (7, 9, 256, 64, 1, 0, 1),       # pointwise variants 6 - 8, the reduction-split forms 1 - 4 of variant 14
    "pw_64_128": (7, 9, 64, 128, 1, 0, 1),       # form 0 of variant 14 (weights in registers) takes C = 64 / 128 only
    "dw_32":     (7, 9, 32, 32, 3, 1, 32),
}


class F32Conv:
    def __init__(self, name, n):
        h, w, c, k, ks, pad, group = F32_CONVS[name]
        self.name, self.n, self.geo = name, n, F32_CONVS[name]
        rng = np.random.default_rng([20281, sorted(F32_CONVS).index(name), n])
        self.x = (rng.random((n, c, h, w)) * 3.0 - 1.0).astype(np.float32)
        self.w = (rng.standard_normal((k, c // group, ks, ks)) * np.sqrt(2.0 / (c // group * ks * ks))).astype(np.float32)
        self.b = (rng.standard_normal(k) * 0.5).astype(np.float32)
        self.want = O.conv_f32_nchw(self.x, self.w, self.b, True, (pad, pad), (1, 1), (1, 1), group)


def f32_conv(name, n):
    if ("f32", name, n) not in _cache:
        _cache["f32", name, n] = F32Conv(name, n)
    return _cache["f32", name, n]


# ---- part A: fully connected layers, fc + softmax, Gemm ----------------------------------------------------------------------------------------
FC_K, FC_N = 2048, 1000
FC_ROWS = (9, 16, 17, 33)              # 9 and 16: the small-batch kernel (one launch with the softmax); 17 and 33: beyond it
FC_F32_ROWS = (17, 33)
GEMM_ROWS = 17
FC_IN_SCALE = 0.031


class FcCase:
    def __init__(self, m):
        rng = np.random.default_rng([20282, m])
        self.m = m
        self.w = (rng.standard_normal((FC_N, FC_K)) * 0.02).astype(np.float32)
        self.b = rng.standard_normal(FC_N).astype(np.float32)
        self.ws = O.weight_scales(self.w)
        self.wq = O.quant_weights(self.w, self.ws)
        self.x = {S8: rand8(rng, (m, FC_K), S8), U8: rand8(rng, (m, FC_K), U8)}
        self.xf = rng.standard_normal((m, FC_K)).astype(np.float32)
        self.want = {S8: O.fc_i8(self.x[S8], self.wq, self.ws, FC_IN_SCALE, self.b), U8: O.fc_i8(self.x[U8], self.wq, self.ws, FC_IN_SCALE, self.b, 0.5)}
        self.want_f32 = O.fc_f32(self.xf, self.w, self.b)


def fc_case(m):
    if ("fc", m) not in _cache:
        _cache["fc", m] = FcCase(m)
    return _cache["fc", m]


# ---- pooling over batch -----------------------------------------------------------------------------------------------------------------------
GPOOL_BATCHES = (GRID_Y_MAX, GRID_Y_MAX + 1)      # launch_pool2d_i8_nhwc puts n on gridDim.y up to 65 535 and takes the generic kernel beyond
GPOOL_HWC = (2, 2, 4)
POOL_N, POOL_HW = 17, (9, 7)
# window, stride, pad, type (0 max, 1 average with the padding, 2 average without), channels
POOL_CASES = [((3, 3), (2, 2), (0, 0), 0, 16), ((3, 3), (2, 2), (1, 1), 0, 6), ((2, 2), (2, 2), (0, 0), 1, 8), ((3, 3), (1, 1), (1, 1), 2, 5),
              ((2, 2), (1, 1), (0, 0), 0, 4)]


def gpool_input(n, dt):
    return rand8(np.random.default_rng([20283, n, dt]), (n,) + GPOOL_HWC, dt)


def pool_input(i, dt):
    rng = np.random.default_rng([20284, i, dt])
    shape = (POOL_N,) + POOL_HW + (POOL_CASES[i][4],)
    return rng.standard_normal(shape).astype(np.float32) if dt == F32 else rand8(rng, shape, dt)


# ---- part B: streaming launchers on their second grid-stride trip ----------------------------------------------------------------------------
def round_half_away(t):
    """roundf of float32 values, in float64 (t + 0.5 is exact there)"""
    t = np.asarray(t, np.float32).astype(np.float64)
    return np.copysign(np.floor(np.abs(t) + 0.5), t)


def ref_quantize_nchw_to_nhwc(x, scale, odt, c_pad):
    """saturate(roundf(x * inv)), inv = 1 / scale (u8: 1 / (scale * 127 / 255)) in f32; channels c .. c_pad - 1 are zero bytes"""
    n, c, h, w = x.shape
    inv = np.float32(1.0) / (np.float32(scale) * (np.float32(127.0) / np.float32(255.0))) if odt == U8 else np.float32(1.0) / np.float32(scale)
    lo, hi = (0, 255) if odt == U8 else (-128, 127)
    q = np.clip(round_half_away(x * inv), lo, hi).astype(NP_DT[odt])
    y = np.zeros((n, h, w, c_pad), NP_DT[odt])
    y[..., :c] = q.transpose(0, 2, 3, 1)
    return y


def ref_dequantize_nhwc_to_nchw(x, scale):
    s = np.float32(scale) * (np.float32(127.0) / np.float32(255.0)) if x.dtype == np.uint8 else np.float32(scale)
    return np.ascontiguousarray((x.astype(np.float32) * s).transpose(0, 3, 1, 2))


def ref_quantize_flat_s8(x, scale):
    return np.clip(round_half_away(x * (np.float32(1.0) / np.float32(scale))), -128, 127).astype(np.int8)


def ref_eltwise_i8(a, b, sa, sb, c0, c1, relu):
    """saturate(roundf((c0 * a) * sa + (c1 * b) * sb)), every product and the sum rounded to f32"""
    f = np.float32
    t = (f(c0) * a.astype(np.float32)) * f(sa) + (f(c1) * b.astype(np.float32)) * f(sb)
    if relu:
        t = np.maximum(t, f(0))
    return np.clip(round_half_away(t), -128, 127).astype(np.int8)


def ref_eltwise_f32(a, b, c0, c1, relu):
    t = np.float32(c0) * a + np.float32(c1) * b
    return np.maximum(t, np.float32(0)) if relu else t


def ref_clipped_relu(x, coef):
    r = np.maximum(x, np.float32(0))
    return np.where(r < np.float32(coef), r, np.float32(coef)).astype(np.float32)


def ref_prelu_nchw(x, slope):
    """x [n, channels, inner]: channel = (i / inner) % channels"""
    return np.where(x > 0, x, x * slope.reshape(1, -1, 1)).astype(np.float32)


def _windows2x2s1(x, ay, ax):
    """the four shifted views of a 2 x 2 / stride-1 window over axes (ay, ax)"""
    def sl(dy, dx):
        ix = [slice(None)] * x.ndim
        ix[ay] = slice(dy, x.shape[ay] - 1 + dy)
        ix[ax] = slice(dx, x.shape[ax] - 1 + dx)
        return x[tuple(ix)]
    return sl(0, 0), sl(0, 1), sl(1, 0), sl(1, 1)


def ref_maxpool2x2s1(x, ay, ax):
    a, b, c, d = _windows2x2s1(x, ay, ax)
    return np.maximum(np.maximum(a, b), np.maximum(c, d))


def ref_avgpool2x2s1_i8_nhwc(x):
    """the 8-bit average: int32 window sum, (float)sum * (1 / 4) in f32, round to nearest even, saturate"""
    a, b, c, d = (v.astype(np.int32) for v in _windows2x2s1(x, 1, 2))
    f = (a + b + c + d).astype(np.float32) * (np.float32(1.0) / np.float32(4.0))
    lo, hi = (0, 255) if x.dtype == np.uint8 else (-128, 127)
    return np.clip(np.rint(f), lo, hi).astype(x.dtype)


def ref_maxpool2x2s1_f32_from_i8(x, scale):
    """dequantise (q * s in f32), 2 x 2 / stride-1 maximum, f32 NCHW"""
    return ref_maxpool2x2s1(ref_dequantize_nhwc_to_nchw(x, scale), 2, 3)


def concat_unit(row_bytes):
    """launch_concat_nhwc: 16 bytes per lane where every row length, offset and the output row length are multiples of 16 (and the
    pointers, which the allocator aligns), else 4, else 1"""
    bits, off = sum(row_bytes), 0
    for r in row_bytes:
        bits |= r | off
        off += r
    return 16 if bits % 16 == 0 else (4 if bits % 4 == 0 else 1)


def _ceil_div(a, b):
    return (a + b - 1) // b


# name -> (launcher, kernel, work items by the launcher's own formula, shape parameters)
def _stream_cases():
    cs = {}

    def add(name, launcher, items, **kw):
        cs[name] = dict(name=name, launcher=launcher, items=int(items), **kw)
    n, c, h, w = 3, 3, 701, 1001
    add("quantize_dword", "launch_quantize_nchw_to_nhwc", n * h * w * (4 >> 2), shape=(n, c, h, w), c_pad=4, odt=S8, scale=0.25)
    n, c, h, w = 2, 3, 593, 591
    add("quantize_bytes", "launch_quantize_nchw_to_nhwc", n * h * w * 3, shape=(n, c, h, w), c_pad=3, odt=U8, scale=0.5)
    add("dequantize", "launch_dequantize_nhwc_to_nchw", n * c * h * w, shape=(n, h, w, c), dt=U8, scale=0.25)
    add("transpose_in", "launch_transpose_nchw_to_nhwc_f32", 1 * 701 * 751 * 4, shape=(1, 3, 701, 751), c_pad=4)
    add("transpose_out", "launch_transpose_nhwc_to_nchw_f32", n * c * h * w, shape=(n, h, w, 4), c=3)
    add("quantize_flat", "launch_quantize_flat_s8", GRID_CAP + 1003, count=GRID_CAP + 1003, scale=0.5)
    cnt = 16 * (GRID_CAP + 777) + 5       # 5 bytes of scalar tail
    add("eltwise_i8", "launch_eltwise_sum_i8", _ceil_div(cnt, 16), count=cnt, sa=0.11, sb=0.043, c0=7.5, c1=-3.25, relu=True)
    cnt = 4 * (GRID_CAP + 777) + 3        # 3 floats of scalar tail
    add("eltwise_f32", "launch_eltwise_sum_f32", _ceil_div(cnt, 4), count=cnt, c0=1.5, c1=-0.75, relu=True)
    add("relu_f32", "launch_relu_f32", _ceil_div(cnt, 4), count=cnt)
    add("clipped_relu_f32", "launch_activation_f32", _ceil_div(cnt, 4), count=cnt, coef=1.7)
    add("prelu_f32", "launch_prelu_f32", 1 * 37 * 56711, shape=(1, 37, 56711))
    px = GRID_CAP // 2 + 501
    for unit, chans in ((16, (16, 32)), (4, (4, 8)), (1, (1, 2))):
        assert concat_unit(chans) == unit
        add("concat_unit%d" % unit, "launch_concat_nhwc", max(px * (r // unit) for r in chans), pixels=px, channels=chans, unit=unit)
    # pooling: 2 x 2 windows at stride 1, no padding (oh = h - 1, ow = w - 1)
    add("pool_i8_avg", "launch_pool2d_i8_nhwc", 2 * 725 * 725 * _ceil_div(6, 4), shape=(2, 726, 726, 6), dt=U8, ptype=1)
    add("pool_i8_max_vec16", "launch_pool2d_i8_nhwc", 2 * 1025 * 1025 * (16 >> 4), shape=(2, 1026, 1026, 16), dt=S8, ptype=0)
    add("pool_f32_nchw", "launch_pool2d_f32", 2 * 592 * 591 * 3, shape=(2, 3, 593, 592), layout="nchw")
    add("pool_f32_nhwc", "launch_pool2d_f32", 2 * 592 * 591 * 3, shape=(2, 593, 592, 3), layout="nhwc")
    add("pool_f32_nhwc_vec4", "launch_pool2d_f32", 3 * 837 * 837 * (4 >> 2), shape=(3, 838, 838, 4), layout="nhwc")
    add("pool_f32_from_i8", "launch_pool2d_f32_from_i8", 2 * 592 * 591 * 3, shape=(2, 593, 592, 3), dt=S8, scale=0.043)
    return cs


STREAM_CASES = _stream_cases()
# pad_channels_i8 is internal to the INT8 C = 3 implicit-GEMM stem path (8 << 16): one 725 x 725 image pads 725 * 725 * 4 = 2 102 500 bytes
PAD_CHANNELS_CASE = dict(name="pad_channels_i8", launcher="launch_pad_channels_i8", items=725 * 725 * 4, shape=(1, 725, 725, 3), k=8)


def stream_rng(name):
    return np.random.default_rng([20285, sorted(STREAM_CASES).index(name)])


def f32_with_ties(rng, shape, scale):
    """f32 values around +-40 quanta of `scale`, every 97th an exact .5 tie (where `scale` is a power of two), every 101st at +-301 quanta: beyond either 8-bit range"""
    x = (rng.standard_normal(shape) * 40.0 * scale).astype(np.float32)
    flat = x.reshape(-1)
    flat[::97] = (np.float32(0.5) + np.round(flat[::97] / np.float32(scale))) * np.float32(scale)
    flat[5::101] = np.where(flat[5::101] >= 0, np.float32(301.0), np.float32(-301.0)) * np.float32(scale)
    return x


def _small(cs):
    """the same case on a slice: spatial sizes 9 x 11 (+ the case's parity), counts of a few thousand with the same scalar tail"""
    cs = dict(cs)
    if "shape" in cs:
        s = list(cs["shape"])
        if cs["name"] == "prelu_f32":
            s[2] = 211
        else:
            ax = (2, 3) if (cs["launcher"] in ("launch_quantize_nchw_to_nhwc", "launch_transpose_nchw_to_nhwc_f32") or cs.get("layout") == "nchw") else (1, 2)
            s[ax[0]], s[ax[1]] = 9, 11
        cs["shape"] = tuple(s)
    if "count" in cs:
        cs["count"] = 4096 + cs["count"] % 16
    if "pixels" in cs:
        cs["pixels"] = 1003
    return cs


def stream_inputs(name, small=False):
    """{argument name: array} of one part-B case (small: the slice tests/test_batch_cpu.py pins the reference on)"""
    cs = _small(STREAM_CASES[name]) if small else STREAM_CASES[name]
    rng = stream_rng(name)
    la = cs["launcher"]
    if la == "launch_quantize_nchw_to_nhwc":
        return {"x": f32_with_ties(rng, cs["shape"], cs["scale"])}
    if la in ("launch_dequantize_nhwc_to_nchw", "launch_pool2d_i8_nhwc", "launch_pool2d_f32_from_i8"):
        return {"x": rand8(rng, cs["shape"], cs["dt"])}
    if la in ("launch_transpose_nchw_to_nhwc_f32", "launch_transpose_nhwc_to_nchw_f32", "launch_pool2d_f32"):
        return {"x": rng.standard_normal(cs["shape"]).astype(np.float32)}
    if la == "launch_quantize_flat_s8":
        return {"x": f32_with_ties(rng, (cs["count"],), cs["scale"])}
    if la == "launch_eltwise_sum_i8":
        return {"a": rand8(rng, (cs["count"],), S8), "b": rand8(rng, (cs["count"],), S8)}
    if la == "launch_eltwise_sum_f32":
        return {"a": rng.standard_normal(cs["count"]).astype(np.float32), "b": rng.standard_normal(cs["count"]).astype(np.float32)}
    if la in ("launch_relu_f32", "launch_activation_f32"):
        return {"x": (rng.standard_normal(cs["count"]) * 2.0).astype(np.float32)}
    if la == "launch_prelu_f32":
        return {"x": rng.standard_normal(cs["shape"]).astype(np.float32), "slope": (rng.standard_normal(cs["shape"][1]) * 0.5).astype(np.float32)}
    if la == "launch_concat_nhwc":
        return {"x%d" % i: rand8(rng, (cs["pixels"], c), S8) for i, c in enumerate(cs["channels"])}
    raise KeyError(name)


def stream_reference(name, a, small=False):
    """the numpy reference of one part-B case on the arrays of stream_inputs"""
    cs = _small(STREAM_CASES[name]) if small else STREAM_CASES[name]
    la = cs["launcher"]
    if la == "launch_quantize_nchw_to_nhwc":
        return ref_quantize_nchw_to_nhwc(a["x"], cs["scale"], cs["odt"], cs["c_pad"])
    if la == "launch_dequantize_nhwc_to_nchw":
        return ref_dequantize_nhwc_to_nchw(a["x"], cs["scale"])
    if la == "launch_transpose_nchw_to_nhwc_f32":
        n, c, h, w = a["x"].shape
        y = np.zeros((n, h, w, cs["c_pad"]), np.float32)
        y[..., :c] = a["x"].transpose(0, 2, 3, 1)
        return y
    if la == "launch_transpose_nhwc_to_nchw_f32":
        return np.ascontiguousarray(a["x"][..., :cs["c"]].transpose(0, 3, 1, 2))
    if la == "launch_quantize_flat_s8":
        return ref_quantize_flat_s8(a["x"], cs["scale"])
    if la == "launch_eltwise_sum_i8":
        return ref_eltwise_i8(a["a"], a["b"], cs["sa"], cs["sb"], cs["c0"], cs["c1"], cs["relu"])
    if la == "launch_eltwise_sum_f32":
        return ref_eltwise_f32(a["a"], a["b"], cs["c0"], cs["c1"], cs["relu"])
    if la == "launch_relu_f32":
        return np.maximum(a["x"], np.float32(0))
    if la == "launch_activation_f32":
        return ref_clipped_relu(a["x"], cs["coef"])
    if la == "launch_prelu_f32":
        return ref_prelu_nchw(a["x"], a["slope"])
    if la == "launch_concat_nhwc":
        return np.concatenate([a["x%d" % i] for i in range(len(cs["channels"]))], axis=-1)
    if la == "launch_pool2d_i8_nhwc":
        return ref_avgpool2x2s1_i8_nhwc(a["x"]) if cs["ptype"] else ref_maxpool2x2s1(a["x"], 1, 2)
    if la == "launch_pool2d_f32":
        return ref_maxpool2x2s1(a["x"], *((2, 3) if cs["layout"] == "nchw" else (1, 2)))
    if la == "launch_pool2d_f32_from_i8":
        return ref_maxpool2x2s1_f32_from_i8(a["x"], cs["scale"])
    raise KeyError(name)


def stream_oracle(name, a):
    """the oracle's own result for the SMALL slice of a part-B case (the transposes and the s8 concat are copies: numpy's own)"""
    cs = _small(STREAM_CASES[name])
    la = cs["launcher"]
    if la == "launch_quantize_nchw_to_nhwc":
        q = O.quant_nchw_to_nhwc(a["x"], cs["scale"], cs["odt"])
        return np.concatenate([q, np.zeros(q.shape[:3] + (cs["c_pad"] - q.shape[3],), q.dtype)], axis=-1)
    if la == "launch_dequantize_nhwc_to_nchw":
        return O.dequant_nhwc_to_nchw(a["x"], cs["scale"])
    if la == "launch_quantize_flat_s8":
        return O.quant_flat_s8(a["x"], cs["scale"])
    if la == "launch_eltwise_sum_i8":
        return O.eltwise_i8(a["a"], a["b"], cs["sa"], cs["sb"], cs["c0"], cs["c1"], cs["relu"])
    if la == "launch_eltwise_sum_f32":
        return O.eltwise_f32(a["a"], a["b"], cs["c0"], cs["c1"], cs["relu"])
    if la == "launch_relu_f32":
        return O.activation_f32(a["x"], 2)
    if la == "launch_activation_f32":
        return O.activation_f32(a["x"], 4, 0.0, cs["coef"])
    if la == "launch_prelu_f32":
        return O.prelu_f32(a["x"], a["slope"], 1)
    if la == "launch_pool2d_i8_nhwc":
        return O.pool_i8_nhwc(a["x"], (2, 2), (1, 1), (0, 0), cs["ptype"])
    if la == "launch_pool2d_f32":
        x = a["x"] if cs["layout"] == "nchw" else a["x"].transpose(0, 3, 1, 2)
        y = O.pool_f32_nchw(x, (2, 2), (1, 1), (0, 0), 0)
        return y if cs["layout"] == "nchw" else np.ascontiguousarray(y.transpose(0, 2, 3, 1))
    if la == "launch_pool2d_f32_from_i8":
        return O.pool_f32_nchw(O.dequant_nhwc_to_nchw(a["x"], cs["scale"]), (2, 2), (1, 1), (0, 0), 0)
    return None
