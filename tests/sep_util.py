"""Separable pairs (depthwise 3x3 + pointwise 1x1 INT8 in one launch, conv_sep.hip): the cases tests/test_gpu_sep.py runs and their
oracle results (O.conv_i8(group=C) followed by O.conv_i8), computed once per case and never modified. No GPU here: tests/test_sep_cpu.py
checks the same cases' preconditions. TEST INFRASTRUCTURE ONLY."""
import numpy as np

from oracle import oracle as O

F32, S8, U8 = O.F32, O.S8, O.U8
NP_DT = {S8: np.int8, U8: np.uint8}

# (n, C, H, W, stride, pad, K)
GEOMETRIES = [
    (2, 32, 9, 7, 1, 1, 64),          # half k-step, W < 16, two images
    (1, 64, 11, 13, 2, 1, 128),       # odd dims at stride 2
    (1, 64, 12, 12, 2, 0, 32),        # pad 0
    (3, 128, 5, 5, 1, 0, 96),         # K % 64 != 0, 9-pixel images
    (1, 256, 17, 18, 1, 1, 256),      # two ragged column tiles
    (1, 512, 14, 14, 2, 1, 1024),     # MobileNet tail
    (2, 1024, 7, 7, 1, 1, 1024),      # MobileNet tail, two images
]
# (in, mid, out, dw relu, pw relu)
DTYPES = [(U8, U8, U8, 1, 1), (S8, S8, S8, 0, 0), (U8, S8, U8, 0, 1), (S8, U8, S8, 1, 0)]
BIASES = [(True, True), (False, True), (True, False), (False, False)]      # (dw, pw): present or absent on each op in turn
IN_SCALE = 0.02
SEP_MAX_CODE = 15

_cache = {}


class Case:
    """One pair: operands, both ops' parameters, the oracle's intermediate and result."""

    def __init__(self, geo, dts, bias, seed, sat=False):
        n, c, h, w, s, p, k = geo
        idt, mdt, odt, relu_dw, relu_pw = dts
        rng = np.random.default_rng(seed)
        self.geo, self.dts, self.bias = geo, dts, bias
        self.x = (rng.integers(0, 256, (n, h, w, c)) if idt == U8 else rng.integers(-128, 128, (n, h, w, c))).astype(NP_DT[idt])
        self.w_dw = (rng.standard_normal((c, 1, 3, 3)) * 0.4).astype(np.float32)
        self.w_pw = (rng.standard_normal((k, c, 1, 1)) * (1.0 / np.sqrt(c))).astype(np.float32)
        self.b_dw = (rng.standard_normal(c) * 0.5).astype(np.float32) if bias[0] else None
        self.b_pw = (rng.standard_normal(k) * 0.5).astype(np.float32) if bias[1] else None
        div = 4.0 if sat else 1.0      # sat: a quarter of the MAXABS scale on both edges
        ws1 = O.weight_scales(self.w_dw)
        wq1 = O.quant_weights(self.w_dw, ws1)
        bp, sc = O.conv_i8_prepare(ws1, self.b_dw, IN_SCALE, 1.0, idt, F32)
        f = O.conv_i8(self.x, wq1, bp, sc, F32, relu_dw, (p, p), (s, s), group=c)
        self.mid_scale = max(float(np.abs(f).max()), 1e-6) / 127.0 / div
        bp, sc = O.conv_i8_prepare(ws1, self.b_dw, IN_SCALE, self.mid_scale, idt, mdt)
        self.mid = O.conv_i8(self.x, wq1, bp, sc, mdt, relu_dw, (p, p), (s, s), group=c)
        ws2 = O.weight_scales(self.w_pw)
        wq2 = O.quant_weights(self.w_pw, ws2)
        bp, sc = O.conv_i8_prepare(ws2, self.b_pw, self.mid_scale, 1.0, mdt, F32)
        f = O.conv_i8(self.mid, wq2, bp, sc, F32, relu_pw)
        self.out_scale = max(float(np.abs(f).max()), 1e-6) / 127.0 / div
        bp, sc = O.conv_i8_prepare(ws2, self.b_pw, self.mid_scale, self.out_scale, mdt, odt)
        self.out = O.conv_i8(self.mid, wq2, bp, sc, odt, relu_pw)


def case(gi, di, sat=False):
    """geometry gi with dtype combination di (the bias pattern follows their sum); cached"""
    key = (gi, di, sat)
    if key not in _cache:
        _cache[key] = Case(GEOMETRIES[gi], DTYPES[di], BIASES[(gi + di) % 4], 20270 + 16 * gi + di + (1000 if sat else 0), sat)
    return _cache[key]


def saturates(y, dt, relu):
    """(saturated, unsaturated) counts of an 8-bit tensor"""
    hi, lo = (255, 0) if dt == U8 else (127, -128)
    sat = np.count_nonzero(y == hi) + (0 if (relu or dt == U8) else np.count_nonzero(y == lo))
    return int(sat), int(np.count_nonzero((y > lo) & (y < hi)))


def identity_dw(c, dt, scale):
    """the operands of a depthwise 3x3 conv whose output IS its input: centre tap 1, w_scale 1, in_scale == out_scale, no bias, no relu
    -> (s8 weights [C, 1, 3, 3], w_scale [C], bias', scale) with the oracle's prepared constants"""
    wq = np.zeros((c, 1, 3, 3), np.int8)
    wq[:, 0, 1, 1] = 1
    ws = np.ones(c, np.float32)
    bp, sc = O.conv_i8_prepare(ws, None, scale, scale, dt, dt)
    return wq, ws, bp, sc
