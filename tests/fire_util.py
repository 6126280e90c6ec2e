"""Concat and SqueezeNet: the float32 numpy restatement of the reference's u8 concat arithmetic, the concat cases tests/test_gpu_fire.py runs,
and the oracle walk of a layer list that holds `concat` entries (oracle/net_oracle.py knows none) composed from O.conv_i8, O.pool_i8_nhwc,
np.concatenate, O.dequant_nhwc_to_nchw + O.pool_f32_nchw and O.softmax_f32 - computed once per input and never modified. No GPU here.
TEST INFRASTRUCTURE ONLY."""
import numpy as np

from oracle import oracle as O

F32, S8, U8 = O.F32, O.S8, O.U8
NP_DT = {F32: np.float32, S8: np.int8, U8: np.uint8}


# ---- the concat operator ----------------------------------------------------------------------------------------------------------------
def concat_multipliers(scales):
    """SaberConcat<X86, AK_INT8>::create (saber/funcs/impl/x86/saber_concat.cpp:163-201): scale_max over the inputs, scale_[i] =
    scale_max / scale_i in float32. Returns (multipliers, output scale)."""
    sc = np.asarray(scales, np.float32)
    return (sc.max() / sc).astype(np.float32), float(sc.max())


def concat_u8_one(x, m):
    """one u8 input through kernel/jit_avx512_core_8bit_concat_kernel.cpp: vpmovzxbd, vcvtdq2ps, vmulps (float32), vcvtps2dq (round to
    nearest even: np.rint), vpmovusdb (unsigned saturation); m == 1: the bytes as they are"""
    m = np.float32(m)
    if m == np.float32(1.0):
        return x.copy()
    p = x.astype(np.float32) * m                      # float32 product, rounded once
    return np.clip(np.rint(p), 0, 255).astype(np.uint8)


def concat_ref(xs, mult=None):
    """xs: arrays [..., c_i] of one dtype; mult: per-input multipliers (u8 only) or None = a copy"""
    if mult is None:
        return np.concatenate(xs, axis=-1)
    assert all(x.dtype == np.uint8 for x in xs)
    return np.concatenate([concat_u8_one(x, m) for x, m in zip(xs, mult)], axis=-1)


def concat_u8_f64(x, m):
    """the same value derived in float64 from the float32 multiplier: (rounded half away from zero, mask of the exact ties). x * m is
    exact in float64 (8 bits x 24 bits); rounding that once to float32 is what vmulps leaves in the register, and the conversion
    to an integer sees nothing else."""
    p = (x.astype(np.float64) * np.float64(np.float32(m))).astype(np.float32).astype(np.float64)
    tie = (p - np.floor(p)) == 0.5
    return np.clip(np.floor(p + 0.5), 0, 255).astype(np.uint8), tie


# (dtype, pixels, channel counts): vector and scalar paths, misaligned offsets, one to eight inputs, more than one block
CONCAT_CASES = {
    "one_input": (S8, 37, [48]),
    "two_vec": (U8, 13 * 13 * 2, [64, 64]),
    "two_vec_f32": (F32, 35, [16, 48]),
    "three_mixed": (U8, 300, [16, 3, 100]),           # the 3 makes every later offset odd
    "three_f32_odd": (F32, 77, [3, 1, 100]),          # 4-byte lanes
    "offset_breaks_vec": (S8, 129, [1, 16, 48]),      # 16-byte rows at offsets 1 and 17
    "eight": (S8, 211, [1, 3, 16, 48, 100, 16, 1, 48]),
    "eight_vec": (U8, 1200, [16, 48, 16, 16, 48, 16, 32, 64]),      # 307 200 bytes: several blocks per input
    "row_not_16": (U8, 50, [16, 100]),                # output row 116 bytes: no 16-byte lanes although input 0 qualifies
}
# u8 multipliers: 1 (copy), below 1, above 1; 0.5 / 1.5 / 2.5 give exact ties at every odd byte, 1.5 and 2.5 and 3 reach the 255 rail
CONCAT_MULTS = {
    "two_vec": [1.0, 1.5],
    "three_mixed": [0.5, 2.5, 1.0],
    "eight_vec": [1.0, 0.5, 1.5, 2.5, 3.0, 0.75, 1.2345678, 0.3333333],
    "row_not_16": [1.5, 0.5],
}


def concat_inputs(name, seed=0):
    dt, pixels, chans = CONCAT_CASES[name]
    rng = np.random.default_rng(4100 + sorted(CONCAT_CASES).index(name) + 100 * seed)
    if dt == F32:
        return [rng.standard_normal((pixels, c)).astype(np.float32) for c in chans]
    lo, hi = (0, 256) if dt == U8 else (-128, 128)
    return [rng.integers(lo, hi, (pixels, c)).astype(NP_DT[dt]) for c in chans]


# ---- a layer list with concat entries, walked with the oracle's operators ---------------------------------------------------------------
def prepare_int8(model):
    prep = {}
    for l in model["spec"]:
        if l["kind"] == "conv":
            w, _ = model["params"][l["name"]]
            ws = O.weight_scales(w)
            prep[l["name"]] = (ws, O.quant_weights(w, ws))
    return prep


def run_int8(model, scales, x, prep=None):
    """x: f32 NCHW. {edge name: tensor} (8-bit edges NHWC) of the framework layer list, one oracle operator per entry; a concat is the
    reference's: output scale = the largest input scale, inputs rescaled by concat_multipliers (all 1 with workloads.calibrate's scales)."""
    scales = dict(scales)
    prep = prep if prep is not None else prepare_int8(model)
    t, dt = {"data": x}, {"data": F32}
    for l in model["spec"]:
        kd, nm = l["kind"], l["name"]
        if kd == "conv":
            _, b = model["params"][nm]
            src, in_dt = t[l["src"]], dt[l["src"]]
            if in_dt == F32:
                src, in_dt = O.quant_nchw_to_nhwc(src, scales[l["src"]], S8), S8
            odt = l.get("odt", U8 if l["relu"] else S8)
            ws, wq = prep[nm]
            bp, sc = O.conv_i8_prepare(ws, b, scales[l["src"]], scales[nm], in_dt, odt)
            t[nm], dt[nm] = O.conv_i8(src, wq, bp, sc, odt, l["relu"], (l["pad"],) * 2, (l["stride"],) * 2, group=l.get("group", 1)), odt
        elif kd == "pool":
            t[nm] = O.pool_i8_nhwc(t[l["src"]], (l["win"],) * 2, (l["stride"],) * 2, (l["pad"],) * 2, l["type"], floor_mode=l.get("floor", False))
            dt[nm], scales[nm] = dt[l["src"]], scales[l["src"]]
        elif kd == "concat":
            srcs = l["srcs"]
            assert len({dt[s] for s in srcs}) == 1
            dt[nm] = dt[srcs[0]]
            if dt[nm] == U8:
                mult, scales[nm] = concat_multipliers([scales[s] for s in srcs])
                t[nm] = concat_ref([t[s] for s in srcs], mult)
            else:
                t[nm] = np.concatenate([t[s] for s in srcs], axis=-1)
        elif kd == "gpool":
            assert not l.get("int8")
            t[nm], dt[nm] = O.pool_f32_nchw(O.dequant_nhwc_to_nchw(t[l["src"]], scales[l["src"]]), None, None, None, 1, global_pool=True), F32
        elif kd == "softmax":
            t[nm], dt[nm] = O.softmax_f32(t[l["src"]].reshape(t[l["src"]].shape[0], -1)), F32
        else:
            raise ValueError("fire_util.run_int8: no %s entries in these models" % kd)
    return t


def run_fp32(model, x):
    """FP32 forward, NCHW, the oracle's naive operators; concat along axis 1"""
    t = {"data": x}
    for l in model["spec"]:
        kd, nm = l["kind"], l["name"]
        if kd == "conv":
            w, b = model["params"][nm]
            t[nm] = O.conv_f32_nchw(t[l["src"]], w, b, l["relu"], (l["pad"],) * 2, (l["stride"],) * 2, group=l.get("group", 1))
        elif kd == "pool":
            t[nm] = O.pool_f32_nchw(t[l["src"]], (l["win"],) * 2, (l["stride"],) * 2, (l["pad"],) * 2, l["type"], floor_mode=l.get("floor", False))
        elif kd == "concat":
            t[nm] = np.concatenate([t[s] for s in l["srcs"]], axis=1)
        elif kd == "gpool":
            t[nm] = O.pool_f32_nchw(t[l["src"]], None, None, None, 1, global_pool=True)
        elif kd == "softmax":
            t[nm] = O.softmax_f32(t[l["src"]].reshape(t[l["src"]].shape[0], -1))
        else:
            raise ValueError("fire_util.run_fp32: no %s entries in these models" % kd)
    return t


def squeezenet_v1_1_macs(hw=224):
    """conv MACs per image counted from the published table alone: conv1 3x3 / 2 -> 64, Fire modules (S, E + E) with 3 / 2 ceil-mode
    pooling in front of fire2, fire4, fire6, conv10 512 -> 1000"""
    def pool(h):
        return -(-(h - 3) // 2) + 1
    h = (hw - 3) // 2 + 1
    total = 3 * 64 * 9 * h * h
    h, cin = pool(h), 64
    for i, (s, e) in enumerate([(16, 64), (16, 64), (32, 128), (32, 128), (48, 192), (48, 192), (64, 256), (64, 256)]):
        total += (cin * s + s * e + 9 * s * e) * h * h
        cin = 2 * e
        if i in (1, 3):
            h = pool(h)
    return total + 512 * 1000 * h * h


# ---- the Fire module as one launch (conv_fire.hip): cases and oracle results, computed once -------------------------------------------------
FIRE_MAX_CODE = 2
IN_SCALE = 0.02
# (C, S, E1, E3, H, W, batch): the smallest at which each thing can go wrong
GEOMETRIES = {
    "a": (16, 16, 16, 16, 5, 7, 2),          # lower rails, W < 16, image index
    "b": (64, 16, 64, 64, 9, 17, 1),         # one-column ragged tile, S = 16
    "c": (128, 32, 128, 128, 13, 13, 2),     # real fire4/5 width at the final size
    "d": (256, 48, 192, 192, 7, 33, 1),      # S not a power of two (K padding), three column tiles
    "e": (512, 64, 256, 256, 13, 13, 1),     # largest LDS / register footprint (fire9)
    "f": (64, 16, 48, 80, 6, 6, 3),          # E1 != E3: the channel offset
    "g1": (32, 16, 16, 16, 1, 1, 1),         # every tap but the centre is padding
    "g2": (32, 16, 16, 16, 2, 3, 1),         # most taps are padding
}
BIASES = [(True, True, True), (False, True, True), (True, False, True), (True, True, False), (False, False, False)]      # (squeeze, e1, e3)
_fire_cache = {}


class FireCase:
    """One module: operands, the three ops' parameters, the oracle's squeeze edge, both expand edges and their concat. zero_x: the input
    all zero bytes and the squeeze biases positive (the case that tells a zero-byte halo from a computed one)."""

    def __init__(self, geo, idt, bias, seed, sat=False, zero_x=False):
        c, s, e1, e3, h, w, n = geo
        rng = np.random.default_rng(seed)
        self.geo, self.idt, self.bias = geo, idt, bias
        x = rng.integers(0, 256, (n, h, w, c)) if idt == U8 else rng.integers(-128, 128, (n, h, w, c))
        self.x = (np.zeros_like(x) if zero_x else x).astype(NP_DT[idt])
        self.w_s = (rng.standard_normal((s, c, 1, 1)) * (1.0 / np.sqrt(c))).astype(np.float32)
        self.w_1 = (rng.standard_normal((e1, s, 1, 1)) * (1.0 / np.sqrt(s))).astype(np.float32)
        self.w_3 = (rng.standard_normal((e3, s, 3, 3)) * (1.0 / np.sqrt(9 * s))).astype(np.float32)
        self.b_s = (rng.standard_normal(s) * 0.5).astype(np.float32) if bias[0] else None
        if zero_x:
            self.b_s = (np.abs(rng.standard_normal(s)) * 0.5 + 0.25).astype(np.float32)
        self.b_1 = (rng.standard_normal(e1) * 0.5).astype(np.float32) if bias[1] else None
        self.b_3 = (rng.standard_normal(e3) * 0.5).astype(np.float32) if bias[2] else None
        div = 4.0 if sat else 1.0      # sat: a quarter of the MAXABS scale on every edge

        def stage(src, src_scale, src_dt, wt, b, pad=0):
            ws = O.weight_scales(wt)
            wq = O.quant_weights(wt, ws)
            bp, sc = O.conv_i8_prepare(ws, b, src_scale, 1.0, src_dt, F32)
            f = O.conv_i8(src, wq, bp, sc, F32, 1, (pad, pad), (1, 1))
            scale = max(float(np.abs(f).max()), 1e-6) / 127.0 / div
            bp, sc = O.conv_i8_prepare(ws, b, src_scale, scale, src_dt, U8)
            return scale, O.conv_i8(src, wq, bp, sc, U8, 1, (pad, pad), (1, 1)), (wq, bp, sc)
        self.s_scale, self.s, _ = stage(self.x, IN_SCALE, idt, self.w_s, self.b_s)
        self.e1_scale, self.e1, _ = stage(self.s, self.s_scale, U8, self.w_1, self.b_1)
        self.e3_scale, self.e3, self.e3_q = stage(self.s, self.s_scale, U8, self.w_3, self.b_3, 1)
        self.y = np.concatenate([self.e1, self.e3], axis=-1)

    def e3_with_computed_halo(self):
        """what a kernel would store that COMPUTED its halo pixels outside the image - squeeze(0) = relu(bias') there - instead of writing
        zero bytes: the 3x3 conv without padding over the squeeze edge extended by one pixel of squeeze(0). For zero_x cases squeeze(0) is
        the squeeze edge's own (constant) pixel."""
        assert not self.x.any()
        wq, bp, sc = self.e3_q
        return O.conv_i8(np.pad(self.s, ((0, 0), (1, 1), (1, 1), (0, 0)), mode="edge"), wq, bp, sc, U8, 1, (0, 0), (1, 1))


def fire_case(name, idt=U8, bi=None, sat=False, zero_x=False):
    """geometry `name`, input dtype idt, bias pattern bi (None: by geometry); cached"""
    key = (name, idt, bi, sat, zero_x)
    if key not in _fire_cache:
        gi = sorted(GEOMETRIES).index(name)
        b = BIASES[(gi if bi is None else bi) % len(BIASES)]
        _fire_cache[key] = FireCase(GEOMETRIES[name], idt, b, 51000 + 16 * gi + (0 if bi is None else bi + 1) + (7 if idt == S8 else 0) + (1000 if sat else 0) +
                                    (2000 if zero_x else 0), sat, zero_x)
    return _fire_cache[key]


def saturation(y):
    """(bytes at the 255 rail, bytes strictly between the rails) of a u8 tensor"""
    return int(np.count_nonzero(y == 255)), int(np.count_nonzero((y > 0) & (y < 255)))
