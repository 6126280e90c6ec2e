"""Directed probes for the INT8 requantisation epilogues: exact ties, both rails and operation order, through every kernel form.

The oracle's sequence (oracle/saber_oracle.c, orc_conv_i8) is
    d = (float)acc;  d += bias';  d *= scale;  relu;  nearbyintf;  saturate
    fused eltwise (RES_ELTWISE):  q = sat_s8(rne(d));  t = c0*q*s0;  t += c1*r*s1;  relu;  roundf;  saturate
    in-place sum (RES_JIT_SUM):   d = sum_scale == 1 ? d + prev : fmaf(prev, sum_scale, d);  relu;  nearbyintf;  saturate
Random data with scales like 0.017 * w_scale / 0.041 essentially never puts d within an ulp of m + 0.5, so a contracted fma, a
reassociated bias, half-away rounding or a clamp at -127 pass the parity tests. These probes put d there on purpose. Plain numpy, no GPU:

  controlled accumulators  every output channel has two non-zero s8 weights, sigma*127 and sigma*1 on the centre tap of one channel pair;
                           a pixel's bytes are (a, b) on every pair, so acc = sigma * (127 a + b) = sigma * t for a chosen integer t.
                           The pixel selects t, the channel selects (sigma, w_scale, bias): an output tensor is their cross product.
  exact scales             w_scale = 0.5 * 2^j and in / out scales of 1 on an s8 side, fl(255/127) on a u8 side give scale = 0.5 and
                           bias' = 2 * bias exactly through the float32 steps of orc_conv_i8_prepare (prepare() restates them), so
                           d = (sigma t + 2 bias) / 2 is an exact half-integer: ties and rails by construction.
  op-order channels        scale and bias' one or a few ulps beside such values: the rounding of d + bias' and of the product then
                           decides the byte; the accumulators at which the reference sequence and each contracted / reassociated form
                           differ are FOUND by search (op_order_search) and put on pixels.
  classes                  counted per probe from the generator's own d (Probe.classes); assert_classes wants every class that applies
                           present, in at least two different positions k % 4 of a lane's four channels.
  emulate(probe, defect)   a float32 numpy model of the epilogue with named defects; tests/test_int8_probe_cpu.py proves on the CPU that
                           the clean model and the oracle agree byte for byte and that every defect changes a byte of every probe family
                           it applies to. tests/test_gpu_int8_probe.py runs the kernels against the oracle on the same probes.

  coefficient pairs        the fused eltwise takes two coefficients, t = c0*q*s0 + c1*r*s1. Beside the four sets with c0 == c1 three modes have
                           c0 != c1 (uneq, neg, zero_res: COEFF_MODES) with products exact in float32; the defects coeff_swap,
                           coeff_conv_for_both and coeff_sign_dropped each change bytes of every such probe they apply to.

On one monotone chain relu, round and saturate commute (round(+-0) = 0, both roundings are monotone), so "relu after the round" and
"saturate before the relu" are identities on a plain convolution and no test can or should separate them there. They are defects where
the chain is not monotone - across the sum of the fused forms - and that is how they are modelled: `relu_across_sum` moves the
convolution's relu behind the eltwise sum, `sat_before_sum` saturates the convolution term before the in-place sum.
"""
import numpy as np

F = np.float32
F32, S8, U8 = 0, 1, 2                      # the oracle's / library's dtype codes
NP_DT = {S8: np.int8, U8: np.uint8}
RANGE = {S8: (-128, 127), U8: (0, 255)}
U_SCALE = F(255.0 / 127.0)                 # a u8 side's scale: fl(s * fl(127/255)) == 1 exactly (asserted below)
HALF_LO = F(np.nextafter(F(0.5), F(0)))    # 0x1.fffffep-2: roundf(t) == trunc(t + copysign(HALF_LO, t))
T_BASE = list(range(11))                   # the accumulators every probe carries: sigma t + bias' spans 11 consecutive integers
BIG = 2.0e6                                # bias' of the "1e6-scale" channels: d = +-1e6, exact in float32

assert F(F(0.5) * U_SCALE) * (F(127.0) / F(255.0)) == F(0.5) and U_SCALE * (F(127.0) / F(255.0)) == F(1.0)


# ---- the float32 arithmetic of the reference -------------------------------------------------------------------------------------------
def prepare(w_scale, bias, in_scale, out_scale, idt, odt):
    """orc_conv_i8_prepare in numpy float32: (bias', scale) per output channel"""
    uf = F(127.0) / F(255.0)
    s_in = np.asarray(w_scale, F) * F(in_scale)
    if idt == U8:
        s_in = s_in * uf
    bp = np.zeros_like(s_in) if bias is None else np.asarray(bias, F) * (F(1.0) / s_in)
    if odt == U8:
        sc = s_in / (F(out_scale) * uf)
    elif odt == S8:
        sc = s_in / F(out_scale)
    else:
        sc = s_in
    return bp.astype(F), sc.astype(F)


def _fma(a, b, c):
    """fl32(a * b + c), the product exact (24 x 24 bits in a double)"""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F)


def _rne(d):
    return np.rint(np.asarray(d, F))


def _roundf(t):
    t64 = np.asarray(t, np.float64)
    return (np.sign(t64) * np.floor(np.abs(t64) + 0.5)).astype(F)


def _sat(v, dt, defect=None):
    """saturate<dt>(float): clamp in the float domain, then cast (v is integral)"""
    lo, hi = RANGE[dt]
    v64 = np.asarray(v, np.float64)
    if defect == "wrap":
        return (v64.astype(np.int64) & 0xff).astype(np.uint8).view(NP_DT[dt])
    if defect == "clamp_m127" and dt == S8:
        lo = -127
    if defect == "u8_no_lower_clamp" and dt == U8:
        return (np.minimum(v64, hi).astype(np.int64) & 0xff).astype(np.uint8)
    return np.clip(v64, lo, hi).astype(NP_DT[dt])


def int_conv(x, wq, pad, stride, depthwise=False):
    """int64 accumulators [N, OH, OW, K] of x NHWC (s8 / u8) with wq OIHW (s8), zero padding; depthwise: wq [C, 1, kh, kw], group = C"""
    N, H, W, C = x.shape
    K, _, kh, kw = wq.shape
    oh, ow = (H + 2 * pad - kh) // stride + 1, (W + 2 * pad - kw) // stride + 1
    xp = np.zeros((N, H + 2 * pad, W + 2 * pad, C), np.int64)
    xp[:, pad:pad + H, pad:pad + W] = x
    w64 = wq.astype(np.int64)
    acc = np.zeros((N, oh, ow, K), np.int64)
    for i in range(kh):
        for j in range(kw):
            if not w64[:, :, i, j].any():
                continue
            xs = xp[:, i:i + stride * (oh - 1) + 1:stride, j:j + stride * (ow - 1) + 1:stride]
            acc += xs * w64[:, 0, i, j] if depthwise else np.einsum("nhwc,kc->nhwk", xs, w64[:, :, i, j])
    return acc


# ---- defects -----------------------------------------------------------------------------------------------------------------------------
ROUND_DEFECTS = ("half_away", "floor_half", "trunc", "conv_roundf")     # conv_roundf: RNE replaced by roundf in the conv (= half_away)
ORDER_DEFECTS = ("fma_bias_scaled", "mul_add", "fma_sum")               # fma(acc, s, b's) | acc*s + b'*s | fma(acc + b', s, 0)
SAT_DEFECTS = ("wrap", "clamp_m127", "u8_no_lower_clamp")
ELT_DEFECTS = ("elt_assoc", "elt_fma", "elt_premul", "elt_rne", "half_identity_05", "relu_across_sum")
SUM_DEFECTS = ("sum_separate", "sat_before_sum")
COEFF_DEFECTS = ("coeff_swap", "coeff_conv_for_both", "coeff_sign_dropped")   # (c1, c0) | (c0, c0) | (|c0|, |c1|) in the fused eltwise
ACC24_DEFECTS = ("acc_cvt_trunc", "acc_cvt_half_up")                    # (float)acc truncating / rounding a tie away from zero
DEFECTS = ROUND_DEFECTS + ORDER_DEFECTS + SAT_DEFECTS + ELT_DEFECTS + SUM_DEFECTS + ACC24_DEFECTS + COEFF_DEFECTS


def _conv_d(acc, bp, sc, defect=None):
    a = np.asarray(acc).astype(F)                       # int -> float: round to nearest even
    if defect in ACC24_DEFECTS:
        a64 = np.asarray(acc).astype(np.float64)        # (exact)
        over = np.abs(a.astype(np.float64)) > np.abs(a64)
        under = np.abs(a.astype(np.float64)) < np.abs(a64)
        if defect == "acc_cvt_trunc":
            a = np.where(over, np.nextafter(a, F(0)), a)
        else:
            tie = under & (np.abs(a64) - np.abs(a.astype(np.float64)) == np.abs(np.nextafter(a, F(np.inf) * np.sign(a)).astype(np.float64) - a64))
            a = np.where(tie, np.nextafter(a, F(np.inf) * np.sign(a)), a)
    if defect == "fma_bias_scaled":
        return _fma(a, sc, bp * sc)
    if defect == "mul_add":
        return a * sc + bp * sc
    if defect == "fma_sum":
        return ((a.astype(np.float64) + bp.astype(np.float64)) * sc.astype(np.float64)).astype(F)
    return (a + bp) * sc


def _round_conv(d, defect=None):
    if defect in ("half_away", "conv_roundf"):
        return _roundf(d)
    if defect == "floor_half":
        return np.floor(d.astype(np.float64) + 0.5).astype(F)
    if defect == "trunc":
        return np.trunc(d)
    return _rne(d)


def _elt_t(q, r, c0, c1, s0, s1, defect=None):
    q, r, c0, c1, s0, s1 = F(q) if np.isscalar(q) else q.astype(F), r.astype(F), F(c0), F(c1), F(s0), F(s1)
    if defect == "coeff_swap":
        c0, c1 = c1, c0
    if defect == "coeff_conv_for_both":
        c1 = c0
    if defect == "coeff_sign_dropped":
        c0, c1 = np.abs(c0), np.abs(c1)
    if defect == "elt_assoc":
        return c0 * (q * s0) + c1 * (r * s1)
    if defect == "elt_fma":
        return _fma(c1 * r, s1, (c0 * q) * s0)
    if defect == "elt_premul":
        return F(c0 * s0) * q + F(c1 * s1) * r
    return (c0 * q) * s0 + (c1 * r) * s1


def _round_elt(t, defect=None):
    if defect == "elt_rne":
        return _rne(t)
    if defect == "half_identity_05":
        return np.trunc(t + np.copysign(F(0.5), t))
    return _roundf(t)


def _sum_d(d, prev, ss, defect=None):
    p = prev.astype(F)
    if F(ss) == F(1.0):
        return d + p
    if defect == "sum_separate":
        return p * F(ss) + d
    return _fma(p, F(ss), d)


# ---- probes ------------------------------------------------------------------------------------------------------------------------------
class Probe:
    """One launch. geo = (N, H, W, C, K, k, pad, stride); x NHWC, wq OIHW s8, per-channel w_scale / bias; mode "conv" | "elt" | "sum".
    elt = (res s8 [N, OH, OW, K], res_relu, (c0, c1), scale_res) - the conv's out_scale is s0; sum = (prev, sum_scale)."""

    def __init__(self, name, geo, idt, odt, relu, x, wq, w_scale, bias, in_scale, out_scale, mode="conv", elt=None, sum_=None, meta=None):
        self.name, self.geo, self.idt, self.odt, self.relu, self.mode = name, geo, idt, odt, bool(relu), mode
        self.x, self.wq, self.w_scale, self.bias = x, wq, np.asarray(w_scale, F), np.asarray(bias, F)
        self.in_scale, self.out_scale, self.elt, self.sum = float(in_scale), float(out_scale), elt, sum_
        self.meta = meta or {}
        self.acc = int_conv(x, wq, geo[6], geo[7], bool(self.meta.get("depthwise")))
        self.bp, self.sc = prepare(self.w_scale, self.bias, in_scale, out_scale, idt, odt)
        assert mode == "conv" or (mode == "elt" and odt == S8) or mode == "sum"

    @property
    def family(self):
        return self.mode

    def d(self, defect=None):
        """the pre-rounding value of the convolution stage (before relu; for "sum": after the sum)"""
        d = _conv_d(self.acc, self.bp, self.sc, defect)
        if self.mode == "sum":
            prev, ss = self.sum
            if defect == "sat_before_sum":
                d = np.clip(d, *RANGE[self.odt])
            d = _sum_d(d, prev, ss, defect)
        return d

    def t(self, defect=None):
        """the pre-rounding value of the eltwise stage (before its relu)"""
        res, res_relu, (c0, c1), s1 = self.elt
        d = self.d(defect)
        if self.relu and defect != "relu_across_sum":
            d = np.maximum(d, F(0))
        q = _sat(_round_conv(d, defect), S8, defect).astype(F)
        return _elt_t(q, res, c0, c1, self.out_scale, s1, defect)

    def applies(self, defect):
        if self.meta.get("kind") == "acc24":
            return defect in ACC24_DEFECTS
        if defect in ACC24_DEFECTS:
            return False
        em = self.meta.get("elt_mode")                    # a fused-eltwise probe carries ONE coefficient set: what it is built to separate
        if defect in ORDER_DEFECTS:
            return bool(self.meta.get("order_channels"))
        if defect in ROUND_DEFECTS:
            return em in (None, "half")
        if defect == "wrap":
            return em in (None, "half", "sum")
        if defect == "clamp_m127":
            return self.odt == S8 and em in (None, "half", "sum") and not (self.relu and self.mode != "elt") and \
                not (self.mode == "elt" and (self.elt[1] or self.relu))
        if defect == "u8_no_lower_clamp":
            return self.odt == U8 and not self.relu and self.mode == "conv"
        if defect == "relu_across_sum":
            return self.relu and em in ("half", "sum")
        if defect == "elt_rne":
            return em == "half"
        if defect == "half_identity_05":
            return em == "below_half"
        if defect in ELT_DEFECTS:
            return em == "order"
        if defect == "coeff_sign_dropped":
            return em == "neg"
        if defect in COEFF_DEFECTS:
            return em in COEFF_MODES
        if defect == "sum_separate":
            return self.mode == "sum" and F(self.sum[1]) not in (F(1.0), F(2.0))
        if defect == "sat_before_sum":
            return self.mode == "sum"
        raise KeyError(defect)

    def classes(self):
        """class name -> boolean mask [N, OH, OW, K], from the generator's own d (and t)"""
        d = self.d().astype(np.float64)
        frac = np.abs(d) - np.floor(np.abs(d))
        tie, m = frac == 0.5, np.floor(np.abs(d))
        inr = np.abs(d) < 1000
        c = {"tie_even_pos": tie & (m % 2 == 0) & (d > 0) & inr, "tie_odd_pos": tie & (m % 2 == 1) & (d > 0) & inr,
             "tie_even_neg": tie & (m % 2 == 0) & (d < 0) & inr, "tie_odd_neg": tie & (m % 2 == 1) & (d < 0) & inr,
             "plus_half": d == 0.5, "minus_half": d == -0.5}
        if self.odt == S8 or self.mode == "elt":
            for v in (126.5, 127.0, 127.5, 128.0, -127.5, -128.0, -128.5, -129.0):
                c["s8_rail_%g" % v] = d == v
            c["s8_big_pos"], c["s8_big_neg"] = d > 1e5, d < -1e5
        else:
            for v in (254.5, 255.0, 255.5, 256.0, -0.5, -1.0):
                c["u8_rail_%g" % v] = d == v
            c["u8_big_neg"] = d < -1e5
        if self.meta.get("order_channels"):
            for dn in ORDER_DEFECTS:
                c["order_" + dn] = self.designated(dn)
        if self.mode == "elt":
            t = self.t().astype(np.float64)
            tf = np.abs(t) - np.floor(np.abs(t))
            c["elt_tie_pos"], c["elt_tie_neg"] = (tf == 0.5) & (t > 0), (tf == 0.5) & (t < 0)
            c["elt_plus_half"], c["elt_minus_half"] = t == 0.5, t == -0.5
            c["elt_rail_hi"], c["elt_rail_lo"] = t >= 127.5, t <= -128.5
            c["elt_q_saturates"] = (d >= 127.5) | (d <= -128.5)
            c["elt_below_half"] = np.abs(t) == float(HALF_LO)
            c["elt_tie_even"], c["elt_tie_odd"] = (tf == 0.5) & (np.floor(np.abs(t)) % 2 == 0), (tf == 0.5) & (np.floor(np.abs(t)) % 2 == 1)
            if self.meta.get("elt_mode") in COEFF_MODES:
                for dn in COEFF_DEFECTS:
                    c[dn] = self.designated(dn)
                c["res_at_rail"] = (self.elt[0] == 127) | (self.elt[0] == -128)
            for dn in ("elt_assoc", "elt_fma", "elt_premul"):
                c["order_" + dn] = self.designated(dn)
        if self.mode == "sum" and F(self.sum[1]) not in (F(1.0), F(2.0)):
            c["order_sum_separate"] = self.designated("sum_separate")
        if self.meta.get("kind") == "acc24":
            c.update(acc24_classes(self))
        return c

    def designated(self, defect):
        """the outputs whose byte the defect changes"""
        return emulate(self, defect) != emulate(self)


def emulate(p, defect=None):
    """the probe's output bytes [N, OH, OW, K] by the float32 model of the epilogue, with one optional named defect"""
    assert defect is None or defect in DEFECTS, defect
    key = ("emu", defect)
    if key in p.meta:
        return p.meta[key]
    if p.mode == "elt":
        t = p.t(defect)
        if p.elt[1] or (defect == "relu_across_sum" and p.relu):
            t = np.maximum(t, F(0))
        out = _sat(_round_elt(t, defect), S8, defect)
    else:
        d = p.d(defect)
        if p.relu or (p.mode == "sum" and p.odt == U8):
            d = np.maximum(d, F(0))
        out = _sat(_round_conv(d, defect), p.odt, defect)
    p.meta[key] = out
    return out


def required_classes(p):
    """the classes that must be present in probe p (each in two positions k % 4)"""
    if p.meta.get("kind") == "acc24":
        return ["acc24_plus1", "acc24_plus3", "acc24_tie"]
    if p.mode == "elt":
        want = {"half": ["elt_tie_pos", "elt_tie_neg", "elt_plus_half", "elt_minus_half", "elt_q_saturates", "tie_even_pos", "tie_odd_pos"] +
                        ["order_" + dn for dn in ORDER_DEFECTS],
                "sum": ["elt_rail_hi", "elt_q_saturates"] + ([] if p.relu else ["elt_rail_lo"]),
                "order": ["order_elt_assoc", "order_elt_fma", "order_elt_premul"],
                "below_half": ["elt_below_half"],
                "uneq": ["elt_tie_pos", "elt_tie_neg", "elt_plus_half", "elt_minus_half", "elt_tie_even", "elt_tie_odd", "elt_rail_hi", "elt_rail_lo",
                         "coeff_swap", "coeff_conv_for_both"],
                "neg": ["elt_tie_pos", "elt_tie_neg", "elt_plus_half", "elt_minus_half", "elt_tie_even", "elt_tie_odd"] + list(COEFF_DEFECTS),
                "zero_res": ["res_at_rail", "elt_q_saturates", "coeff_swap", "coeff_conv_for_both"]}[p.meta["elt_mode"]]
        if p.elt[1]:           # a relu behind the sum: no negative byte leaves the launch
            want = [w for w in want if w not in ("elt_tie_neg", "elt_minus_half", "elt_rail_lo")] if p.meta["elt_mode"] in COEFF_MODES else want
        return want
    want = ["tie_even_pos", "tie_odd_pos", "plus_half"]
    if p.mode == "conv":
        want += ["tie_even_neg", "tie_odd_neg", "minus_half"] + ["order_" + dn for dn in ORDER_DEFECTS]
        if p.odt == S8:
            want += ["s8_rail_%g" % v for v in (126.5, 127.0, 127.5, 128.0, -127.5, -128.0, -128.5, -129.0)] + ["s8_big_pos", "s8_big_neg"]
        else:
            want += ["u8_rail_%g" % v for v in (254.5, 255.0, 255.5, 256.0, -0.5, -1.0)] + ["u8_big_neg"]
    else:
        hi = 127 if p.odt == S8 else 255
        want += ["%s_rail_%g" % ("s8" if p.odt == S8 else "u8", v) for v in (hi - 0.5, hi, hi + 0.5, hi + 1)]
        if F(p.sum[1]) == F(1.0):
            want += ["order_" + dn for dn in ORDER_DEFECTS]
        elif F(p.sum[1]) != F(2.0):      # an inexact sum_scale: prev * s is no integer, so no exact tie exists; what it is for is the fmaf
            want = ["order_sum_separate"]
    return want


def class_counts(p):
    return {k: int(v.sum()) for k, v in p.classes().items()}


def assert_classes(*probes):
    """every required class present in two lane positions k % 4; several probes: the passes of one case (a pooled launch shows the
    channels of one sign per pass), counted together on the outputs meta["keep"] marks"""
    cls = [p.classes() for p in probes]
    for name in required_classes(probes[0]):
        lanes, n = set(), 0
        for p, cl in zip(probes, cls):
            m = cl[name] & p.meta["keep"] if "keep" in p.meta else cl[name]
            lanes |= {int(k) % 4 for k in np.nonzero(m.any(axis=(0, 1, 2)))[0]}
            n += int(m.sum())
        assert len(lanes) >= 2, ("probe %s: class %s in %d lane positions k %% 4 (%d outputs)" % (probes[0].name, name, len(lanes), n))


def max_pool_3x3s2(y):
    """3x3 / 2 max pooling of y NHWC without padding, ceil shapes, windows clipped at the border: what the stem launch applies"""
    N, H, W, K = y.shape
    ph, pw = -(-(H - 3) // 2) + 1, -(-(W - 3) // 2) + 1
    out = np.full((N, ph, pw, K), np.iinfo(y.dtype).min, y.dtype)
    for i in range(3):
        for j in range(3):
            v = y[:, i::2, j::2][:, :ph, :pw]
            np.maximum(out[:, :v.shape[1], :v.shape[2]], v, out=out[:, :v.shape[1], :v.shape[2]])
    return out


def pooled_keep(p):
    """meta["keep"] of a pooled probe at the pooled shape: output (py, px) shows conv output (2 py + 1, 2 px + 1)"""
    return p.meta["keep"][:, 1::2, 1::2, :]


def f32_image_of(x):
    """an f32 NCHW image that the quantise-on-entry step (saturate(roundf(v / in_scale)), in_scale 1) turns into the s8 bytes x NHWC:
    on every other pixel the value is the exact tie q - 0.5 sign(q), which must round AWAY from zero to q"""
    q = x.astype(np.float32).transpose(0, 3, 1, 2).copy()
    N, C, H, W = q.shape
    tie = ((np.arange(H)[:, None] + np.arange(W)[None, :]) % 2 == 0)[None, None] & (q != 0)
    return np.where(tie, q - np.float32(0.5) * np.sign(q), q).astype(np.float32)


# ---- generation --------------------------------------------------------------------------------------------------------------------------
def _io_scales(idt, odt):
    return float(U_SCALE if idt == U8 else 1.0), float(U_SCALE if odt == U8 else 1.0)


def _pow2_channels(odt):
    """(sigma, bias') of the exact channels: d = (sigma t + bias') / 2 for t = 0 .. 10"""
    ch = [(1, -5.0), (-1, 5.0),                       # d = -2.5 .. 2.5: ties of both parities and signs, +-0.5
          (1, 248.0), (-1, 258.0),                    # 124 .. 129 from below and from above: the upper s8 rail
          (-1, -250.0), (1, -260.0),                  # -125 .. -130: the lower s8 rail
          (1, 504.0), (-1, 514.0),                    # 252 .. 257: the upper u8 rail
          (1, BIG), (-1, -BIG), (1, -1.0)]            # +-1e6; -0.5 .. 4.5
    return ch


def _order_candidates(idt, odt):
    """(w_scale, bias) candidates of the op-order channels. scale = 0.75 * 2^j (two mantissa bits: acc * scale is exact and n * scale is a
    tie for n = 2 mod 4) and bias' = n0 + delta with delta between a third and a half ulp of acc + bias': the reference's add rounds
    delta away and lands ON the tie, a form that does not round the sum (or scales the bias first) lands above it."""
    s_i, s_o = _io_scales(idt, odt)
    out = []
    for w in (0.75, 0.375, 1.5):
        s_in = prepare(np.array([w]), None, s_i, s_o, idt, F32)[1][0]
        for e in (6, 5, 7):
            for base in (2.0, 6.0, 1.0, 3.0):
                b0 = F(F(base + 27.0 / 64.0 * 2.0 ** (e - 23)) * s_in)
                for u in (0, 1, -1, 2, -2):          # bias' = bias * fl(1 / s_in) is off by an ulp or two: try the neighbours
                    b = b0
                    for _ in range(abs(u)):
                        b = np.nextafter(b, F(np.inf if u > 0 else -np.inf))
                    out.append((F(w), b))
    return out


def op_order_search(idt, odt, relu, t_max=400, n_extra=4):
    """By search over the candidate channels and the accumulators t in [0, t_max]: up to three channels (one per w_scale), each with
    one t at which the reference sequence and EACH of ORDER_DEFECTS round to different, unsaturated bytes.
    Returns ([(sigma, w_scale, bias)], [t])."""
    s_i, s_o = _io_scales(idt, odt)
    t = np.arange(t_max + 1)
    lo, hi = RANGE[odt]
    chans, chosen = {}, []
    for ws, b in _order_candidates(idt, odt):
        if float(ws) in chans:
            continue
        bp, sc = prepare(np.array([ws]), np.array([b]), s_i, s_o, idt, odt)

        def byte(defect):
            d = _conv_d(t, bp, sc, defect)
            return np.clip(_rne(np.maximum(d, F(0)) if relu else d), lo, hi), d
        ref, d = byte(None)
        common = (d > lo + 1) & (d < hi - 1)
        for dn in ORDER_DEFECTS:
            common &= byte(dn)[0] != ref
        if not common.any():
            continue
        hit = t[common].tolist()
        again = [v for v in hit if v in chosen]
        if not again and len(chosen) >= n_extra:
            continue
        chans[float(ws)] = (1, float(ws), float(b))
        if not again:
            chosen.append(hit[0])
    assert chans, ("no op-order channel separates the three forms", idt, odt, relu)
    return list(chans.values()), sorted(chosen)


def _weights(geo, sigma):
    """wq [K, C, k, k]: sigma*127 and sigma*1 on the centre tap of channel pair k % (C // 2)"""
    N, H, W, C, K, k, pad, stride = geo
    wq = np.zeros((K, C, k, k), np.int8)
    kk = np.arange(K)
    pair = kk % (C // 2)
    wq[kk, 2 * pair, k // 2, k // 2] = 127 * np.asarray(sigma)
    wq[kk, 2 * pair + 1, k // 2, k // 2] = np.asarray(sigma)
    return wq


def out_hw(geo):
    N, H, W, C, K, k, pad, stride = geo
    return (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1


def _image(geo, idt, tvals, rng, pool_bg=None):
    """x NHWC: output pixel p reads (a, b) with 127 a + b = tvals[p % len] on every channel pair under its centre tap.
    pool_bg (a 3x3 / 2 max pooling follows): only the outputs at odd (y, x) - the centre of exactly one pooling window each - carry
    tvals, every other output has the accumulator pool_bg."""
    N, H, W, C, K, k, pad, stride = geo
    assert pad == k // 2
    oh, ow = out_hw(geo)
    if pool_bg is None:
        P = N * oh * ow
        tv = np.asarray(tvals)[np.arange(P) % len(tvals)].reshape(N, oh, ow)
    else:
        tv = np.full((N, oh, ow), pool_bg, np.int64)
        n_c = tv[:, 1::2, 1::2].size
        tv[:, 1::2, 1::2] = np.asarray(tvals)[np.arange(n_c) % len(tvals)].reshape(tv[:, 1::2, 1::2].shape)
    lo, hi = RANGE[idt]
    a = np.clip(np.rint(tv / 127.0).astype(np.int64) if idt == S8 else tv // 127, lo, hi)
    b = tv - 127 * a
    assert (b >= lo).all() and (b <= hi).all(), "accumulator out of reach"
    x = np.zeros((N, H, W, C), np.int64)
    if C % 2:
        x[..., C - 1] = rng.integers(lo, hi + 1, (N, H, W))      # a channel no weight reads
    iy, ix = np.arange(oh) * stride, np.arange(ow) * stride
    x[:, iy[:, None], ix[None, :], 0:C - C % 2:2] = a[..., None]
    x[:, iy[:, None], ix[None, :], 1:C - C % 2:2] = b[..., None]
    return x.astype(NP_DT[idt]), tv


def _channel_params(K, chans):
    """channel k gets chans[k % L]; an odd L puts every entry on both parities of k, so on two positions k % 4"""
    L = len(chans)
    assert L % 2 == 1 and K >= 2 * L, (L, K)
    idx = np.arange(K) % L
    sig = np.array([chans[i][0] for i in idx])
    ws = np.array([chans[i][1] for i in idx], F)
    b = np.array([chans[i][2] for i in idx], F)
    return sig, ws, b


def conv_probe(name, geo, idt, odt, relu, seed=0, pool=None):
    """the plain convolution's probe: exact channels (ties, rails, +-1e6) and searched op-order channels.
    pool = "bgmin" | "bgmax": a 3x3 / 2 max pooling follows (the stem launch). A window shows its largest byte, so the probed outputs sit
    on the window centres and the others hold the smallest (bgmin) or largest (bgmax) accumulator: under bgmin every channel with
    sigma = +1 shows its probed bytes through the pooling, under bgmax every channel with sigma = -1; meta["keep"] marks them."""
    rng = np.random.default_rng(seed)
    s_i, s_o = _io_scales(idt, odt)
    order, extra = op_order_search(idt, odt, relu)
    chans = [(s, 0.5, bp / 2.0) for s, bp in _pow2_channels(odt)] + order
    while len(chans) % 2 == 0 or len(chans) < 13:
        chans.append(order[len(chans) % len(order)])
    sig, ws, b = _channel_params(geo[4], chans)
    tvals = T_BASE + extra
    x, tv = _image(geo, idt, tvals, rng, None if pool is None else (min(tvals) if pool == "bgmin" else max(tvals)))
    meta = {"t": tvals, "order_channels": order, "acc24": "out of reach: see acc24_probe"}
    if pool is not None:
        oh, ow = out_hw(geo)
        keep = np.zeros((geo[0], oh, ow, geo[4]), bool)
        keep[:, 1::2, 1::2, :] = (sig > 0) if pool == "bgmin" else (sig < 0)
        meta.update(pool=pool, keep=keep)
    return Probe(name, geo, idt, odt, relu, x, _weights(geo, sig), ws, b, s_i, s_o, meta=meta)


def gpool_probe(name, geo, idt, odt, relu, seed=0):
    """a convolution whose output also goes through the fused global average pooling (rne(sum over the pixels * (1 / count)), count a
    power of two): the channels' bias' are FOUND by search so that the sum of a channel's output bytes is count * (m + 0.5) - an exact
    tie of the pooled value - for both parities of m and, on s8, both signs."""
    rng = np.random.default_rng(seed)
    s_i, s_o = _io_scales(idt, odt)
    N, H, W, C, K, k, pad, stride = geo
    oh, ow = out_hw(geo)
    cnt = oh * ow
    assert cnt & (cnt - 1) == 0 and N == 1
    tv = np.asarray(T_BASE)[np.arange(cnt) % len(T_BASE)]
    lo, hi = RANGE[odt]
    found = {}
    for s in (1, -1):
        for bp in range(-80, 560):
            d = (s * tv + bp).astype(F) * F(0.5)
            y = np.clip(_rne(np.maximum(d, F(0)) if relu else d), lo, hi)
            tot = int(y.sum())
            if tot % cnt == cnt // 2 and lo * cnt < tot < hi * cnt:
                found.setdefault((tot // cnt) % 2 + 2 * (tot < 0), []).append((s, 0.5, bp / 2.0))
    chans = [c for key in sorted(found) for c in found[key][:3]]
    assert len(found) >= (2 if relu or odt == U8 else 4), ("pooled ties of both parities and signs", sorted(found))
    chans = chans[:11] if len(chans) % 2 == 0 and len(chans) > 11 else chans
    if len(chans) % 2 == 0:
        chans.append((1, 0.5, 0.0))
    sig, ws, b = _channel_params(K, chans)
    x, _ = _image(geo, idt, T_BASE, rng)
    return Probe(name, geo, idt, odt, relu, x, _weights(geo, sig), ws, b, s_i, s_o, meta={"kind": "gpool", "t": T_BASE})


def dw_probe(name, geo, idt, odt, relu, seed=0):
    """depthwise 3x3 (group = C = K): one weight sigma on the centre tap, the pixel's byte is the accumulator t itself (t <= 127)"""
    N, H, W, C, K, k, pad, stride = geo
    assert C == K and k == 3 and pad == 1
    s_i, s_o = _io_scales(idt, odt)
    order, extra = op_order_search(idt, odt, relu, t_max=127)
    chans = [(s, 0.5, bp / 2.0) for s, bp in _pow2_channels(odt)] + order + order[:1]
    sig, ws, b = _channel_params(K, chans)
    oh, ow = out_hw(geo)
    tvals = T_BASE + extra
    tv = np.asarray(tvals)[np.arange(N * oh * ow) % len(tvals)].reshape(N, oh, ow)
    x = np.zeros((N, H, W, C), np.int64)
    x[:, (np.arange(oh) * stride)[:, None], (np.arange(ow) * stride)[None, :], :] = tv[..., None]
    wq = np.zeros((C, 1, 3, 3), np.int8)
    wq[:, 0, 1, 1] = sig
    return Probe(name, geo, idt, odt, relu, x.astype(NP_DT[idt]), wq, ws, b, s_i, s_o,
                 meta={"t": tvals, "order_channels": order, "depthwise": True, "acc24": "out of reach: nine taps"})


COEFF_MODES = ("uneq", "neg", "zero_res")                 # c0 != c1: what a swapped, merged or sign-dropped coefficient pair changes
ELT_MODES = ("half", "sum", "order", "below_half") + COEFF_MODES
ELT_COEFFS = {"half": ((1.0, 1.0), 0.5, 0.5), "sum": ((2.0, 2.0), 0.5, 0.5), "order": ((float(F(1.0 / 0.06)),) * 2, 0.05, 0.043),
              "below_half": ((1.0, 1.0), float(HALF_LO), float(HALF_LO)),
              "uneq": ((1.0, 3.0), 0.5, 0.5), "neg": ((1.0, -1.0), 0.5, 0.5), "zero_res": ((2.0, 0.0), 0.5, 0.5)}      # mode -> ((c0, c1), s0, s1)
# 2 t of the uneq mode, t = (q + 3 r) / 2: +-0.5, ties of both parities and signs, both rails from inside and outside, integers
_UNEQ_2T = np.array([1, -1, 3, -3, 5, -5, 255, 257, -257, -259, 7, -7, 253, -255, 0, 2])


def _uneq_residual(q, mix):
    """r with q + 3 r = the first entry of _UNEQ_2T from position mix on that q reaches exactly (the table holds every residue mod 3)"""
    tt = _UNEQ_2T[(mix[..., None] + np.arange(16)) % 16]                # [..., 16]: the table rotated to start at mix
    num = tt - q[..., None]
    ok = (num % 3 == 0) & (num // 3 >= -128) & (num // 3 <= 127)
    first = ok.argmax(axis=-1)
    r = np.take_along_axis(num, first[..., None], axis=-1)[..., 0] // 3
    return np.where(ok.any(axis=-1), r, 0)


def _elt_order_table(c0, c1, s0, s1):
    """disc[q + 128] = the residual bytes r at which the reference eltwise and each reassociated / contracted form round differently"""
    q, r = np.meshgrid(np.arange(-128, 128), np.arange(-128, 128), indexing="ij")
    ref = np.clip(_roundf(_elt_t(q, r, c0, c1, s0, s1)), -128, 127)
    out = {}
    for dn in ("elt_assoc", "elt_fma", "elt_premul"):
        out[dn] = np.clip(_roundf(_elt_t(q, r, c0, c1, s0, s1, dn)), -128, 127) != ref
    return out


def elt_probe(name, geo, idt, relu, res_relu, elt_mode, seed=0):
    """conv (-> s8, scale 0.5: q's own rounding has ties) + fused eltwise; the residual bytes are chosen per output from q.
    half: c s0 = c s1 = 0.5, t = (q + r) / 2 - ties go half away;  sum: c s = 1, t = q + r in [-256, 254] - both rails;
    order: the network's kind of coefficients (1 / 0.06, 0.05, 0.043), (q, r) found by search;  below_half: s = 0x1.fffffep-2, t = +-s.
    c0 != c1 (s0 = s1 = 0.5, every product exact):  uneq: (1, 3), t = (q + 3 r) / 2 - halves of both parities and signs, both rails;
    neg: (1, -1), t = (q - r) / 2 - a dropped sign;  zero_res: (2, 0), t = q under residual bytes at the rails - the residual must not leak."""
    rng = np.random.default_rng(seed)
    s_i = float(U_SCALE if idt == U8 else 1.0)
    (c, c1), s0, s1 = ELT_COEFFS[elt_mode]
    chans = [(s, float(F(0.5) * F(s0)), float(F(bp / 2.0) * (F(0.5) * F(s0)) * F(2.0))) for s, bp in _pow2_channels(S8)]
    order, extra = [], []
    if elt_mode == "half":          # out_scale = 0.5: w_scale / 2 and bias / 2 give the (bias', scale) the search saw, exactly
        order, extra = op_order_search(idt, S8, relu)
        order = [(s, w / 2.0, b_ / 2.0) for s, w, b_ in order]
        chans += order + order[:1]
    n_exact = len(_pow2_channels(S8))
    sig, ws, b = _channel_params(geo[4], chans)
    x, tv = _image(geo, idt, T_BASE + extra, rng)
    p = Probe(name, geo, idt, S8, relu, x, _weights(geo, sig), ws, b, s_i, s0, mode="elt",
              elt=(None, bool(res_relu), (c, c1), s1), meta={"elt_mode": elt_mode, "t": T_BASE + extra, "order_channels": order})
    d = p.d()
    q = np.clip(_rne(np.maximum(d, F(0)) if relu else d), -128, 127).astype(np.int64)
    N, oh, ow, K = q.shape
    mix = (np.arange(N * oh * ow).reshape(N, oh, ow, 1) + 3 * np.arange(K)) % 16
    if elt_mode == "half":
        target = np.array([1, -1, 3, -3, 5, -5, 253, 254, -255, -256, -257, 0, 2, 7, -7, 251])[mix]
        r = target - q
        is_order = (np.arange(K) % len(chans)) >= n_exact      # an op-order channel: q + r even, so that q + 1 moves the output
        r = np.where(is_order, 100 - q, r)
    elif elt_mode == "sum":
        target = np.array([254, -256, 127, 128, -128, -129, 255, -257, 200, -200, 129, -130, 0, 1, -1, 126])[mix]
        r = target - q
    elif elt_mode == "below_half":
        r = np.where(mix % 2 == 0, 1, -1) - q
    elif elt_mode == "uneq":
        r = _uneq_residual(q, mix + np.zeros_like(q))
    elif elt_mode == "neg":                 # q - r = 2 t
        r = q - np.array([1, -1, 3, -3, 5, -5, 253, 254, -255, -256, -257, 0, 2, 7, -7, 251])[mix]
    elif elt_mode == "zero_res":            # any r but q itself (a swapped pair gives r), half of them on a rail
        r = np.array([127, -128, 100, -100, 127, -128, 1, -1, 127, -128, 64, -64, 127, -128, 3, -3])[mix] + np.zeros_like(q)
        r = np.where(r == q, -1 - q, r)
    else:
        tab = _elt_order_table(c, c, s0, s1)
        r = rng.integers(-128, 128, q.shape)
        names = list(tab)
        for n_ in range(N):
            for y_ in range(oh):
                for x_ in range(ow):
                    for k_ in range(K):
                        cand = np.nonzero(tab[names[int(mix[n_, y_, x_, 0] + k_) % 3]][q[n_, y_, x_, k_] + 128])[0]
                        if len(cand):
                            r[n_, y_, x_, k_] = cand[(y_ + x_ + k_) % len(cand)] - 128
    res = np.clip(r, -128, 127).astype(np.int8)
    p.elt = (res, bool(res_relu), (c, c1), s1)
    return p


SUM_SCALE_NE1 = float(F(0.5) * (F(1) + F(2.0 ** -23)))      # not 1 and not exact: fmaf(prev, s, d) and prev*s + d differ


def sum_probe(name, geo, idt, odt, rdt, relu, sum_scale, seed=0):
    """conv accumulating onto the bytes already in the output (dtype rdt): prev is chosen per output so that the sum is a tie or a rail
    (sum_scale 1), or - found by search over the 256 bytes - so that the reference's fmaf and a separate multiply and add differ."""
    rng = np.random.default_rng(seed)
    s_i, s_o = _io_scales(idt, odt)
    chans = [(s, 0.5, bp / 2.0) for s, bp in _pow2_channels(odt)]
    order, extra = [], []
    if F(sum_scale) == F(1.0):
        order, extra = op_order_search(idt, odt, relu)
        chans += order + order[:1]
    n_exact = len(_pow2_channels(odt))
    sig, ws, b = _channel_params(geo[4], chans)
    x, tv = _image(geo, idt, T_BASE + extra, rng)
    p = Probe(name, geo, idt, odt, relu, x, _weights(geo, sig), ws, b, s_i, s_o, mode="sum", sum_=(None, sum_scale),
              meta={"t": T_BASE + extra, "rdt": rdt, "order_channels": order})
    d = _conv_d(p.acc, p.bp, p.sc)
    N, oh, ow, K = d.shape
    hi = 127 if odt == S8 else 255
    mix = (np.arange(N * oh * ow).reshape(N, oh, ow, 1) + 3 * np.arange(K)) % 16
    target = np.array([0.5, 1.5, 2.5, 3.5, hi - 0.5, hi, hi + 0.5, hi + 1, -0.5, -1.5, -2.5, -127.5, -128.5, -128, -129, 4.5])[mix]
    lo_r, hi_r = RANGE[rdt]
    if F(sum_scale) == F(2.0):          # fmaf(prev, 2, d) is exact: d + 2 prev keeps d's half, ties and rails after a sum with sum_scale != 1
        prev = np.clip(np.floor((target - d.astype(np.float64)) / 2.0), lo_r, hi_r)
    elif F(sum_scale) == F(1.0):
        prev = np.clip(np.floor(target - d.astype(np.float64)), lo_r, hi_r)
        prev = np.where((np.arange(K) % len(chans)) >= n_exact, 2, prev)      # an op-order channel: an even prev keeps the tie's parity
    else:
        prev = np.clip(np.floor((target - d.astype(np.float64)) / sum_scale), lo_r, hi_r)
        cand = np.arange(lo_r, hi_r + 1).astype(F)
        dd = d[..., None]
        relu_ = relu or odt == U8
        a_ = _fma(cand, F(sum_scale), dd)
        b_ = cand * F(sum_scale) + dd
        if relu_:
            a_, b_ = np.maximum(a_, F(0)), np.maximum(b_, F(0))
        diff = np.clip(_rne(a_), *RANGE[odt]) != np.clip(_rne(b_), *RANGE[odt])
        has = diff.any(axis=-1)
        first = diff.argmax(axis=-1) + lo_r
        prev = np.where(has, first, prev)
    p.sum = (prev.astype(NP_DT[rdt]), sum_scale)
    return p


def acc24_probe(name, geo, odt, seed=0):
    """|acc| = 2^24 + 1 and 2^24 + 3 (u8 input, a 3x3 kernel over C >= 64): (float)acc must round to nearest even - 2^24 and 2^24 + 4.
    bias' = -2^24 + 1 / + 3 and scale 0.5 turn the converted value into the tie 0.5 (-> 0) resp. 3.5 (-> 4); a conversion that truncates
    or rounds half up gives other bytes. Dense weights sigma*127 with one weight sigma*1, the whole image holds two byte values."""
    N, H, W, C, K, k, pad, stride = geo
    assert k == 3 and pad == 1 and stride == 1 and C >= 64 and H >= 3 and W >= 3
    n127 = 9 * C - 1
    x = np.zeros((N, H, W, C), np.int64)
    wq = np.full((K, C, k, k), 127, np.int64)
    wq[:, 0, 1, 1] = 1
    # interior outputs of row y: 127 * (sum of the other bytes) + x[centre, 0]; choose bytes per image ROW so that rows differ
    # acc = 2^24 + e: 127 * S + b with S = 132104, b = 9 + (e - 1)  (2^24 + 1 = 127 * 132104 + 9)
    S = 132104
    base, rem = divmod(S, n127)
    assert base + 1 <= 255
    flat = np.full(n127, base, np.int64)
    flat[:rem] += 1
    x[:] = base
    sig = np.where(np.arange(K) % 3 == 2, -1, 1)
    # one designated output pixel per image: (1, 1); its window is written explicitly, channel 0 of the centre holds b
    win = np.zeros((3, 3, C), np.int64)
    win.reshape(-1)[np.arange(9 * C) != (4 * C)] = flat
    meta = {"kind": "acc24", "pixels": []}
    for n in range(N):
        for j, e in enumerate((1, 3)):
            cx = 1 + 3 * j
            if cx + 1 >= W:
                continue
            w_ = win.copy()
            w_[1, 1, 0] = 9 + (e - 1)
            x[n, 0:3, cx - 1:cx + 2] = w_
            meta["pixels"].append((n, 1, cx, e))
    wq = (wq * sig[:, None, None, None]).astype(np.int8)
    s_i, s_o = _io_scales(U8, odt)
    # bias' = -sigma 2^24 + {1, 3}: with scale 0.5, RNE of 2^24 + 1 -> 2^24 -> d = 0.5 | 1.5; of 2^24 + 3 -> 2^24 + 4 -> d = 2.5 | 3.5
    bsel = np.where((np.arange(K) // 3) % 2 == 0, 1.0, 3.0)
    bias_p = -sig * 2.0 ** 24 + sig * bsel
    p = Probe(name, geo, U8, odt, False, x.astype(np.uint8), wq, np.full(K, 0.5, F), (bias_p / 2.0).astype(F), s_i, s_o, meta=meta)
    assert np.array_equal(p.bp.astype(np.float64), bias_p)
    return p


def acc24_classes(p):
    a = np.abs(p.acc)
    d = p.d().astype(np.float64)
    frac = np.abs(d) - np.floor(np.abs(d))
    return {"acc24_plus1": a == 2 ** 24 + 1, "acc24_plus3": a == 2 ** 24 + 3, "acc24_tie": (a > 2 ** 24) & (frac == 0.5) & (np.abs(d) < 200)}


def describe(p, idx):
    """the classes output idx = (n, y, x, k) of probe p belongs to, its d (and t): what a failing byte was probing"""
    idx = tuple(int(i) for i in idx)
    names = [k for k, v in p.classes().items() if v[idx]]
    s = "classes %s, acc %d, d %.9g" % (names or ["-"], int(p.acc[idx]), float(p.d()[idx]))
    if p.mode == "elt":
        s += ", t %.9g, residual %d" % (float(p.t()[idx]), int(p.elt[0][idx]))
    if p.mode == "sum":
        s += ", prev %d" % int(p.sum[0][idx])
    return s


def oracle_bytes(p):
    """the oracle's output of probe p [N, OH, OW, K], computed once; asserts prepare() against orc_conv_i8_prepare"""
    from oracle import oracle as O
    key = "oracle"
    if key in p.meta:
        return p.meta[key]
    bp, sc = O.conv_i8_prepare(p.w_scale, p.bias, p.in_scale, p.out_scale, p.idt, p.odt)
    assert np.array_equal(bp, p.bp) and np.array_equal(sc, p.sc), (p.name, "prepare() differs from orc_conv_i8_prepare")
    pad, st = (p.geo[6],) * 2, (p.geo[7],) * 2
    if p.mode == "conv":
        y = O.conv_i8(p.x, p.wq, bp, sc, p.odt, int(p.relu), pad, st, group=p.geo[3] if p.meta.get("depthwise") else 1)
    elif p.mode == "elt":
        res, res_relu, (c0, c1), s1 = p.elt
        y = O.eltwise_i8(O.conv_i8(p.x, p.wq, bp, sc, O.S8, int(p.relu), pad, st), res, p.out_scale, s1, c0, c1, res_relu)
    else:
        prev, ss = p.sum
        rp = O.Residual(O.RES_JIT_SUM, 0, ss, p.meta["rdt"], 0, 0, 0, 0)
        y = O.conv_i8(p.x, p.wq, bp, sc, p.odt, int(p.relu), pad, st, residual=rp, out_init=prev.view(NP_DT[p.odt]))
    p.meta[key] = y
    return y


# ---- the cases both test files run -------------------------------------------------------------------------------------------------------
# (N, H, W, C, K, k, pad, stride): the smallest shapes the kernel families accept
GEOMETRIES = {
    "pw_k64": (1, 8, 8, 64, 64, 1, 0, 1),
    "pw_k72": (1, 8, 8, 64, 72, 1, 0, 1),        # K % 16 != 0: the generic epilogue's vector store
    "pw_k34": (1, 8, 8, 64, 34, 1, 0, 1),        # K % 4 != 0: its scalar stores
    "c3x3": (1, 9, 9, 64, 64, 3, 1, 1),          # halo kernels; |acc| > 2^24 in reach
    "img3x3": (2, 10, 9, 128, 64, 3, 1, 1),      # image-resident slabs
    "stem": (1, 30, 30, 3, 64, 7, 3, 2),
    "imgres1x1": (1, 4, 4, 1024, 64, 1, 0, 1),   # the image-resident kernel (whole image in LDS, <= 64 pixels): res5's channel shapes only
    "imgres3x3": (1, 4, 7, 512, 64, 3, 1, 1),
}
DW_GEOMETRIES = {"s1": (1, 7, 9, 32, 32, 3, 1, 1), "s2": (1, 7, 9, 32, 32, 3, 1, 2)}      # depthwise: C = K = group
STEM_POOL_IMAGES = [(30, 30), (18, 23)]          # stem conv + 3x3 / 2 max pooling in one launch: conv output 15x15 / 9x12
for _h, _w in STEM_POOL_IMAGES:
    GEOMETRIES["stempool%dx%d" % (_h, _w)] = (1, _h, _w, 3, 64, 7, 3, 2)
DT_NAME = {S8: "s8", U8: "u8"}
CONV_COMBOS = [(i, o, r) for i in (S8, U8) for o in (S8, U8) for r in (0, 1)]
ELT_COMBOS = [(i, r, rr, m) for i in (S8, U8) for r, rr in ((0, 0), (0, 1), (1, 1)) for m in ELT_MODES]
SUM_COMBOS = [(i, o, rd, r, ss) for i, o, rd, r in ((U8, U8, S8, 1), (U8, S8, U8, 0), (S8, S8, S8, 0), (S8, U8, U8, 1)) for ss in (1.0, SUM_SCALE_NE1, 2.0)]
FUSED_GEOMETRIES = ("pw_k64", "pw_k72", "pw_k34", "c3x3", "img3x3", "imgres1x1", "imgres3x3")      # the 1x1 and 3x3 single-conv cases


# the persistent stage launch (C, N, H, W): C = 64 on two column tiles with a ragged one, four / three tile rows with a ragged last row
STAGE_PROBE_SHAPES = [(256, 2, 7, 9), (128, 1, 5, 13), (64, 2, 7, 9), (64, 1, 5, 24)]


def stage_block_probes(shape):
    """[(which conv of the block carries the probe, probe name, geometry)] of one stage shape: what tests/test_gpu_int8_probe.py's
    test_chain_stage_probes_each_epilogue_of_its_first_block builds (a stage's 3x3 convs write u8)"""
    C, N, H, W = shape
    out = [(0, "conv/chain3/%su8/relu1" % DT_NAME[i], (N, H, W, C, C, 3, 1, 1)) for i in (U8, S8)]
    out += [(1, "elt/chain3/u8/relu0_res%d/%s" % (rr, m), (N, H, W, C, 4 * C, 1, 0, 1)) for rr in (0, 1) for m in ELT_MODES]
    return out + [(2, "conv/chain3b/s8u8/relu1", (N, H, W, 4 * C, C, 1, 0, 1))]


GPOOL_NAMES = ["gpool/imgres1x1/%s%s/relu%d" % (DT_NAME[i], DT_NAME[o], r) for i in (S8, U8) for o, r in ((S8, 0), (S8, 1), (U8, 1))]


def group_list():
    """group name -> [probe names]: one test per group, in both files"""
    g = {}
    for gn in GEOMETRIES:
        if gn.startswith("stempool"):
            continue
        g["conv/" + gn] = ["conv/%s/%s%s/relu%d" % (gn, DT_NAME[i], DT_NAME[o], r) for i, o, r in CONV_COMBOS]
    for gn in FUSED_GEOMETRIES:
        for i in (S8, U8):
            g["elt/%s/%s" % (gn, DT_NAME[i])] = ["elt/%s/%s/relu%d_res%d/%s" % (gn, DT_NAME[i], r, rr, m) for i2, r, rr, m in ELT_COMBOS if i2 == i]
        g["sum/" + gn] = ["sum/%s/%s%s%s/relu%d/ss%s" % (gn, DT_NAME[i], DT_NAME[o], DT_NAME[rd], r, {1.0: "1", 2.0: "2"}.get(ss, "ne1"))
                          for i, o, rd, r, ss in SUM_COMBOS]
    for hw in STEM_POOL_IMAGES:
        for i in (S8, U8):
            g["stempool/%dx%d/%s" % (hw + (DT_NAME[i],))] = ["conv/stempool%dx%d/%s%s/relu%d/%s" % (hw + (DT_NAME[i], DT_NAME[o], o == U8, bg))
                                                              for o in (S8, U8) for bg in ("bgmin", "bgmax")]
    for gn in DW_GEOMETRIES:
        g["dw/" + gn] = ["dw/%s/%s%s/relu%d" % (gn, DT_NAME[i], DT_NAME[o], r) for i, o, r in CONV_COMBOS]
    for gn in ("c3x3", "img3x3", "imgres3x3"):
        g["acc24/" + gn] = ["acc24/%s/%s" % (gn, DT_NAME[o]) for o in (S8, U8)]
    return g


_CODE = {v: k for k, v in DT_NAME.items()}
_cache = {}


def build(name, geo=None):
    """the probe of a name from group_list() (geo: another geometry under the same recipe - the fused forms' tests); cached, never modified"""
    key = (name, geo)
    if key in _cache:
        return _cache[key]
    f = name.split("/")
    geo = (DW_GEOMETRIES if f[0] == "dw" else GEOMETRIES)[f[1]] if geo is None else geo
    seed = int.from_bytes(name.encode(), "little") % (2 ** 31)
    if f[0] == "conv":
        p = conv_probe(name, geo, _CODE[f[2][:2]], _CODE[f[2][2:]], int(f[3][-1]), seed, f[4] if len(f) > 4 else None)
    elif f[0] == "elt":
        p = elt_probe(name, geo, _CODE[f[2]], int(f[3][4]), int(f[3][-1]), f[4], seed)
    elif f[0] == "sum":
        p = sum_probe(name, geo, _CODE[f[2][:2]], _CODE[f[2][2:4]], _CODE[f[2][4:]], int(f[3][-1]), {"ss1": 1.0, "ss2": 2.0}.get(f[4], SUM_SCALE_NE1), seed)
    elif f[0] == "dw":
        p = dw_probe(name, geo, _CODE[f[2][:2]], _CODE[f[2][2:]], int(f[3][-1]), seed)
    elif f[0] == "gpool":
        p = gpool_probe(name, geo, _CODE[f[2][:2]], _CODE[f[2][2:]], int(f[3][-1]), seed)
    else:
        p = acc24_probe(name, geo, _CODE[f[2]], seed)
    _cache[key] = p
    return p


# ---- the streaming ops: eltwise, quantise, average pooling, fc ---------------------------------------------------------------------------
ELT_SETS = dict(ELT_COEFFS)               # name -> ((c0, c1), s0, s1): elt_probe's coefficient sets


def eltwise_grid():
    """(a, b): every pair of s8 bytes, [256, 256] each - the eltwise op's whole domain per coefficient set"""
    return tuple(np.ascontiguousarray(v.astype(np.int8)) for v in np.meshgrid(np.arange(-128, 128), np.arange(-128, 128), indexing="ij"))


def eltwise_model(a, b, c, s0, s1, relu, defect=None):
    """c: the pair (c0, c1)"""
    t = _elt_t(a.astype(np.int64), b.astype(np.int64), c[0], c[1], s0, s1, defect)
    if relu:
        t = np.maximum(t, F(0))
    return _sat(_round_elt(t, defect), S8, defect)


def quant_values(out_dtype):
    """(x f32 NCHW [1, 4, 5, 19], scale): x * (1 / scale') is exactly m + 0.5 (both signs, even and odd m), +-HALF_LO, the rails and
    +-1e6; the quantisers round half AWAY from zero (roundf). scale' = scale on s8, scale * 127/255 on u8: 1 here."""
    hi = 127 if out_dtype == S8 else 255
    v = [0.5, -0.5, 1.5, -1.5, 2.5, -2.5, 3.5, float(HALF_LO), -float(HALF_LO), 0.0, -0.0, 1.0, float(np.nextafter(F(1.5), F(0))),
         float(np.nextafter(F(2.5), F(9))), hi - 0.5, hi, hi + 0.5, hi + 1.0, -127.5, -128.0, -128.5, -129.0, 1e6, -1e6, 126.5, 254.5,
         8388607.5, -8388607.5, 100.5, -100.5, 4.5, -4.5, 63.5, -63.5, 0.25, -0.75, 31.5, 32.5]
    x = np.resize(np.array(v, F), (1, 4, 5, 19)).copy()
    x[0, 1] = -x[0, 1]
    return x, float(U_SCALE if out_dtype == U8 else 1.0)


def quant_model(x, out_dtype, defect=None):
    """saturate(roundf(x * inv)), inv = 1 for quant_values' scales"""
    r = _rne(x) if defect == "elt_rne" else (np.trunc(x + np.copysign(F(0.5), x)) if defect == "half_identity_05" else _roundf(x))
    return _sat(r, out_dtype, defect)


POOL_WINDOWS = [((2, 2), (2, 2), (0, 0), 1), ((3, 3), (1, 1), (1, 1), 2), ((3, 3), (2, 2), (1, 1), 1), ((7, 7), (1, 1), (3, 3), 2),
                ((2, 2), (1, 1), (0, 0), 2)]      # (window, stride, pad, type): 1 = average over the window, 2 = over its valid part


def pool_image(dt, H=8, W=8):
    """x NHWC [2, H, W, 16]: a checkerboard of (a_c, b_c) with a_c + b_c odd, so every window with an even count of cells sums to
    count * (m + 0.5): sum * fl(1 / count) is a tie (count a power of two) or an ulp beside one (6, 12, 20 ...)."""
    pairs = [(1, 0), (2, 1), (3, 2), (4, 3), (127, 126), (126, 125), (100, 1), (64, 63)] if dt == U8 else \
            [(1, 0), (2, 1), (0, -1), (-1, -2), (-3, 2), (127, 126), (-128, -127), (-127, -126)]
    if dt == U8:
        pairs += [(255, 254), (254, 253), (255, 0), (200, 1), (129, 128), (128, 127), (5, 0), (6, 1)]
    else:
        pairs += [(3, 2), (-2, -3), (127, -128), (-4, 1), (5, 4), (-5, -6), (100, -99), (-100, 99)]
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    even = ((yy + xx) % 2 == 0)[None, :, :, None]
    a = np.array([p_[0] for p_ in pairs])[None, None, None, :]
    b = np.array([p_[1] for p_ in pairs])[None, None, None, :]
    x = np.where(even, a, b) * np.ones((2, 1, 1, 1), np.int64)
    x[1] = np.where(even, b, a)[0]
    return x.astype(NP_DT[dt])


def pool_model(x, win, stride, pad, ptype, out_hw_, global_pool=False, defect=None):
    """average pooling of x NHWC as the reference does it: int32 sum, * fl(1 / count), round half even, saturate"""
    N, H, W, C = x.shape
    dt = S8 if x.dtype == np.int8 else U8
    if global_pool:
        win, stride, pad, out_hw_ = (H, W), (H, W), (0, 0), (1, 1)
    oh, ow = out_hw_
    out = np.zeros((N, oh, ow, C), NP_DT[dt])
    for y in range(oh):
        for x_ in range(ow):
            hs, ws = max(y * stride[0] - pad[0], 0), max(x_ * stride[1] - pad[1], 0)
            he, we = min(y * stride[0] - pad[0] + win[0], H), min(x_ * stride[1] - pad[1] + win[1], W)
            cnt = (he - hs) * (we - ws) if ptype == 2 else win[0] * win[1]
            s = x[:, hs:he, ws:we].astype(np.int64).sum(axis=(1, 2)).astype(F)
            f = s / F(cnt) if defect == "pool_divide" else s * (F(1.0) / F(cnt))
            out[:, y, x_] = _sat(_roundf(f) if defect == "half_away" else _rne(f), dt)
    return out


def fc_probe(M, K, N, idt):
    """(x [M, K], wq [N, K], w_scale [N], bias [N], in_scale, out_scale): controlled accumulators (weights 127 and 1 on two columns, as
    the convolutions'; row m has the accumulator 9973 + 797 m, negated on every third output) under scales and biases with full mantissas.
    The s8-operand epilogue is (float)acc * scale + bias in two roundings - fc_model's defect "fma" contracts it -, the u8-operand one
    scale * (float)(acc + (int)(bias / scale)) - its defect "bias_float" adds the bias in float instead."""
    lo, hi = RANGE[idt]
    x = np.zeros((M, K), np.int64)
    wq = np.zeros((N, K), np.int8)
    n = np.arange(N)
    sig = np.where(n % 3 == 2, -1, 1)
    col = 2 * (n * 37 % (K // 2))
    wq[n, col], wq[n, col + 1] = 127 * sig, sig
    tv = 9973 + 797 * np.arange(M)
    a = np.clip(tv // 127, 0, hi)
    x[:, 0::2] = a[:, None]
    x[:, 1::2] = (tv - 127 * a)[:, None]
    ws = (F(0.3137) * (F(1) + F(2.0 ** -20) * n.astype(F)) / F(1024)).astype(F)
    bias = ((n % 7 - 3).astype(F) * F(0.7301) + F(1.0) / F(3.0)).astype(F)
    return x.astype(NP_DT[idt]), wq, ws, bias, 0.031, (0.5 if idt == U8 else 1.0)


def fc_model(x, wq, ws, bias, in_scale, out_scale, defect=None):
    """the INT8 fc's f32 output [M, N] as the reference computes it (orc_fc_i8_s8in / orc_fc_i8_u8in), with one optional defect"""
    acc = x.astype(np.int64) @ wq.astype(np.int64).T
    if x.dtype == np.int8:
        sc = ws * F(in_scale)
        a = acc.astype(F)
        return _fma(a, sc, bias) if defect == "fma" else a * sc + bias
    sc = (F(in_scale) * ws) / F(out_scale)
    if defect == "bias_float":
        return sc * acc.astype(F) + bias
    acc = acc + (bias / sc).astype(np.int64)          # (int)(bias / scale): truncation
    return np.where(sc == F(1.0), acc.astype(F), sc * acc.astype(F))
