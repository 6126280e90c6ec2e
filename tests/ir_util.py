"""Inverted-residual blocks (1x1 expand + depthwise 3x3 + 1x1 project [+ eltwise] INT8 in one launch, conv_ir.hip): the cases
tests/test_gpu_ir.py runs and their oracle results - O.conv_i8 -> O.conv_i8(group=Ce) -> O.conv_i8 [-> O.eltwise_i8 with the block's
input] - computed once per case and never modified. No GPU here. TEST INFRASTRUCTURE ONLY."""
import numpy as np

from oracle import oracle as O

F32, S8, U8 = O.F32, O.S8, O.U8
NP_DT = {S8: np.int8, U8: np.uint8}
IR_MAX_CODE = 7
IN_SCALE = 0.02

# (Cin, Ce, Cout, H, W, stride, residual, batch)
GEOMETRIES = {
    "a": (16, 96, 16, 5, 7, 1, True, 2),          # W < 16, odd dims
    "b": (24, 144, 24, 9, 17, 1, True, 1),        # every channel tail at once, one-column ragged tile
    "d": (24, 144, 32, 9, 11, 2, False, 2),       # odd dims at stride 2
    "e": (32, 192, 64, 14, 14, 2, False, 1),
    "f": (64, 384, 64, 14, 14, 1, True, 3),
    "g": (96, 576, 96, 10, 33, 1, True, 1),       # several row tiles and three column tiles
    "h": (160, 960, 320, 7, 7, 1, False, 1),      # largest LDS and register footprint
    "i": (8, 48, 8, 3, 3, 1, True, 1),            # the lower rails of the accepted range
}
# dtype and epilogue variants: (x dtype, residual, project relu -> u8, eltwise relu); a residual needs s8 input and an s8 project conv
VARIANTS = [(S8, True, 0, 0), (S8, True, 0, 1), (S8, False, 0, 0), (S8, False, 1, 0), (U8, False, 0, 0), (U8, False, 1, 0)]
BIASES = [(True, True, True), (False, True, True), (True, False, True), (True, True, False), (False, False, False)]      # (expand, dw, project)

_cache = {}


def _quant(w):
    ws = O.weight_scales(w)
    return ws, O.quant_weights(w, ws)


class Case:
    """One block: operands, the three ops' parameters, the oracle's two inner edges and result. variant = (idt, residual, project relu,
    eltwise relu); zero_x: the input all zero bytes and the expand biases positive (the zero-padding case); pair: the project eltwise's
    coefficients as multiples of c = 1 / y_scale (None: (c, c)) - .coeffs holds the pair, .coeff its first entry."""

    def __init__(self, geo, variant, bias, seed, sat=False, zero_x=False, pair=None):
        cin, ce, cout, h, w, s, _, n = geo
        idt, res, p_relu, e_relu = variant
        assert not res or (idt == S8 and cin == cout and s == 1 and not p_relu)
        rng = np.random.default_rng(seed)
        self.geo, self.variant, self.bias, self.res = geo, variant, bias, res
        self.idt, self.odt, self.p_relu, self.e_relu = idt, (U8 if p_relu else S8), p_relu, e_relu
        x = rng.integers(0, 256, (n, h, w, cin)) if idt == U8 else rng.integers(-128, 128, (n, h, w, cin))
        self.x = (np.zeros_like(x) if zero_x else x).astype(NP_DT[idt])
        self.w_e = (rng.standard_normal((ce, cin, 1, 1)) * (1.0 / np.sqrt(cin))).astype(np.float32)
        self.w_d = (rng.standard_normal((ce, 1, 3, 3)) * 0.4).astype(np.float32)
        self.w_p = (rng.standard_normal((cout, ce, 1, 1)) * (1.0 / np.sqrt(ce))).astype(np.float32)
        self.b_e = (rng.standard_normal(ce) * 0.5).astype(np.float32) if bias[0] else None
        if zero_x:
            self.b_e = (np.abs(rng.standard_normal(ce)) * 0.5 + 0.25).astype(np.float32)
        self.b_d = (rng.standard_normal(ce) * 0.5).astype(np.float32) if bias[1] else None
        self.b_p = (rng.standard_normal(cout) * 0.5).astype(np.float32) if bias[2] else None
        div = 4.0 if sat else 1.0      # sat: a quarter of the MAXABS scale on every edge

        def stage(src, src_scale, src_dt, w, b, odt, relu, pad=0, stride=1, group=1):
            ws, wq = _quant(w)
            bp, sc = O.conv_i8_prepare(ws, b, src_scale, 1.0, src_dt, F32)
            f = O.conv_i8(src, wq, bp, sc, F32, relu, (pad, pad), (stride, stride), group=group)
            scale = max(float(np.abs(f).max()), 1e-6) / 127.0 / div
            bp, sc = O.conv_i8_prepare(ws, b, src_scale, scale, src_dt, odt)
            return scale, O.conv_i8(src, wq, bp, sc, odt, relu, (pad, pad), (stride, stride), group=group)
        self.e_scale, self.e = stage(self.x, IN_SCALE, idt, self.w_e, self.b_e, U8, 1)
        self.d_scale, self.d = stage(self.e, self.e_scale, U8, self.w_d, self.b_d, U8, 1, 1, s, ce)
        self.p_scale, self.p = stage(self.d, self.d_scale, U8, self.w_p, self.b_p, self.odt, p_relu)
        self.y, self.y_scale = self.p, self.p_scale
        if res:
            m0, m1 = (1.0, 1.0) if pair is None else pair
            f = np.float32(m0) * np.float32(self.p_scale) * self.p.astype(np.float32) + np.float32(m1) * np.float32(IN_SCALE) * self.x.astype(np.float32)
            self.y_scale = max(float(np.abs(np.maximum(f, 0) if e_relu else f).max()), 1e-6) / 127.0 / div
            c = np.float32(1.0 / self.y_scale)
            self.coeffs = (float(np.float32(m0) * c), float(np.float32(m1) * c))
            self.coeff = self.coeffs[0]
            self.y = O.eltwise_i8(self.p, self.x, self.p_scale, IN_SCALE, self.coeffs[0], self.coeffs[1], bool(e_relu))


def case(name, vi=None, sat=False, zero_x=False, pair=None):
    """geometry `name` with variant vi (None: the geometry's own residual flag, s8 input, no relus); cached"""
    geo = GEOMETRIES[name]
    variant = (S8, geo[6], 0, 0) if vi is None else VARIANTS[vi]
    key = (name, variant, sat, zero_x, pair)
    if key not in _cache:
        gi = sorted(GEOMETRIES).index(name)
        bi = (gi + (0 if vi is None else vi + 1)) % len(BIASES)
        _cache[key] = Case(geo, variant, BIASES[bi], 30270 + 16 * gi + (0 if vi is None else vi + 1) + (1000 if sat else 0) + (2000 if zero_x else 0),
                           sat, zero_x, pair)
    return _cache[key]


def saturates(y, dt, relu):
    """(saturated high, saturated low or None where the type / relu has no low rail of its own, unsaturated) counts of an 8-bit tensor"""
    hi, lo = (255, 0) if dt == U8 else (127, -128)
    low = None if (relu or dt == U8) else int(np.count_nonzero(y == lo))
    return int(np.count_nonzero(y == hi)), low, int(np.count_nonzero((y > lo) & (y < hi)))


def identity_expand(c, dt, scale):
    """a 1x1 conv c -> c whose u8 output IS its u8 input: identity weights, w_scale 1, in_scale == out_scale, no bias (relu changes nothing)"""
    assert dt == U8
    wq = np.zeros((c, c, 1, 1), np.int8)
    wq[np.arange(c), np.arange(c), 0, 0] = 1
    return wq, np.ones(c, np.float32)


def identity_dw(c):
    """a depthwise 3x3 conv whose u8 output IS its u8 input: centre tap 1, w_scale 1, in_scale == out_scale, no bias"""
    wq = np.zeros((c, 1, 3, 3), np.int8)
    wq[:, 0, 1, 1] = 1
    return wq, np.ones(c, np.float32)


def mobilenet_v2_macs():
    """conv + fc MACs per 224 x 224 image, counted from the (t, c, n, s) table alone"""
    hw, cin, total = 112, 32, 3 * 32 * 9 * 112 * 112
    for t, c, n, s in [(1, 16, 1, 1), (6, 24, 2, 2), (6, 32, 3, 2), (6, 64, 4, 2), (6, 96, 3, 1), (6, 160, 3, 2), (6, 320, 1, 1)]:
        for i in range(n):
            st = s if i == 0 else 1
            ce = cin * t
            if t != 1:
                total += cin * ce * hw * hw
            hw = (hw - 1) // st + 1
            total += 9 * ce * hw * hw + ce * c * hw * hw
            cin = c
    return total + 320 * 1280 * hw * hw + 1280 * 1000
