"""Expected values for the resize op (anakin_amd/csrc/resize.hip): a numpy restatement of the reference's saber_resize.cpp in float32, a
float64 evaluation of the same coordinates, the case list of tests/test_resize_cpu.py and tests/test_gpu_resize.py, and the FPN-style op
list of the executor tests.

resize_ref follows the reference step by step. Per axis, with `in` / `out` the sizes and o the output index, every step rounded to float32:
  mode 0 BILINEAR_ALIGN     s = float(in - 1) / float(out - 1); f = float(o) * s;  i0 = (int)f, i1 = i0 + (i0 < in - 1)
  mode 1 BILINEAR_NO_ALIGN  s = float(in) / float(out); f = max(s * (float(o) + 0.5f) - 0.5f, 0);  taps as mode 0
  mode 2 RESIZE_CUSTOM      s = 1.f / scale (scale = float(out) / float(in) where sizes are given); f = float(o) * s; i1 = i0 + 1, a tap >= in reads 0
  mode 3 NEAREST_ALIGN      s as mode 0; the one tap (int)(double(float(o) * s) + 0.5)
frac = f - float(i0); the weights are double products rounded to float once; y = ((w00 * tl + w01 * tr) + w10 * bl) + w11 * br in float32.
numpy rounds every float32 array operation to float32 and fuses nothing, which is exactly that."""
import numpy as np

BILINEAR_ALIGN, BILINEAR_NO_ALIGN, RESIZE_CUSTOM, NEAREST_ALIGN = 0, 1, 2, 3
F32 = np.float32


def case(n, c, h, w, mode, out_h=-1, out_w=-1, scale_h=0.0, scale_w=0.0):
    return dict(n=n, c=c, h=h, w=w, mode=mode, out_h=out_h, out_w=out_w, scale_h=float(scale_h), scale_w=float(scale_w))


def sizes_given(cs):
    return cs["out_h"] != -1 and cs["out_w"] != -1


def out_hw(cs):
    """Resize::compute_output_shape: the sizes where both are given, else floor(in * scale) with the product in float32"""
    if sizes_given(cs):
        return cs["out_h"], cs["out_w"]
    return int(np.floor(F32(cs["h"]) * F32(cs["scale_h"]))), int(np.floor(F32(cs["w"]) * F32(cs["scale_w"])))


def axis_table(mode, n_in, n_out, scale, given):
    """(i0, i1, frac) of every output index along one axis: int32, int32, float32"""
    o = np.arange(n_out, dtype=F32)
    if mode in (BILINEAR_ALIGN, NEAREST_ALIGN):
        assert n_out > 1, "the reference divides by out - 1"
        s = F32(n_in - 1) / F32(n_out - 1)
    elif mode == BILINEAR_NO_ALIGN:
        s = F32(n_in) / F32(n_out)
    else:
        sc = F32(n_out) / F32(n_in) if given else F32(scale)
        assert sc > 0
        s = F32(1.0) / sc
    if mode == NEAREST_ALIGN:
        p = o * s
        idx = np.maximum((p.astype(np.float64) + 0.5).astype(np.int32), 0)
        return idx, idx.copy(), np.zeros(n_out, F32)
    if mode == BILINEAR_NO_ALIGN:
        f = s * (o + F32(0.5))
        f = f - F32(0.5)
        f = np.maximum(f, F32(0.0))
    else:
        f = o * s
    assert f.dtype == F32
    i0 = f.astype(np.int32)
    i1 = i0 + 1 if mode == RESIZE_CUSTOM else i0 + (i0 < n_in - 1)
    frac = f - i0.astype(F32)
    assert frac.dtype == F32
    return i0, i1.astype(np.int32), frac


def tables(cs):
    oh, ow = out_hw(cs)
    g = sizes_given(cs)
    return axis_table(cs["mode"], cs["h"], oh, cs["scale_h"], g), axis_table(cs["mode"], cs["w"], ow, cs["scale_w"], g)


def _taps(x, th, tw):
    """the four taps of every output pixel, [n, c, oh, ow] each; a tap beyond the input reads 0 (in x's dtype)"""
    h, w = x.shape[2], x.shape[3]
    (h0, h1, _), (w0, w1, _) = th, tw
    okh, okw = h1 < h, w1 < w
    h1c, w1c = np.minimum(h1, h - 1), np.minimum(w1, w - 1)
    z = x.dtype.type(0)
    tl = x[:, :, h0][:, :, :, w0]
    tr = np.where(okw[None, None, None, :], x[:, :, h0][:, :, :, w1c], z)
    bl = np.where(okh[None, None, :, None], x[:, :, h1c][:, :, :, w0], z)
    br = np.where((okh[:, None] & okw[None, :])[None, None], x[:, :, h1c][:, :, :, w1c], z)
    return tl, tr, bl, br


def _weights64(th, tw):
    fh = th[2].astype(np.float64)[:, None]
    fw = tw[2].astype(np.float64)[None, :]
    return (1.0 - fh) * (1.0 - fw), fw * (1.0 - fh), fh * (1.0 - fw), fw * fh


def resize_ref(x_nchw, cs):
    """float32, the reference's order of operations; x [n, c, h, w] -> [n, c, oh, ow]"""
    x = np.ascontiguousarray(x_nchw, F32)
    th, tw = tables(cs)
    if cs["mode"] == NEAREST_ALIGN:
        return np.ascontiguousarray(x[:, :, th[0]][:, :, :, tw[0]])
    tl, tr, bl, br = _taps(x, th, tw)
    w00, w01, w10, w11 = (v.astype(F32)[None, None] for v in _weights64(th, tw))
    y = ((w00 * tl + w01 * tr) + w10 * bl) + w11 * br
    assert y.dtype == F32
    return np.ascontiguousarray(y)


def resize_f64(x_nchw, cs):
    """the same coordinates (the float32 tables), weights and sums in float64"""
    x = np.asarray(x_nchw, np.float64)
    th, tw = tables(cs)
    if cs["mode"] == NEAREST_ALIGN:
        return x[:, :, th[0]][:, :, :, tw[0]]
    tl, tr, bl, br = _taps(x, th, tw)
    w00, w01, w10, w11 = (v[None, None] for v in _weights64(th, tw))
    return w00 * tl + w01 * tr + w10 * bl + w11 * br


def sum_ref(r, b, c0, c1, relu):
    """eltwise_sum_f32_kernel's expression on float32 arrays: fadd(fmul(c0, r), fmul(c1, b)), relu as a clamp at 0"""
    t = F32(c0) * r.astype(F32) + F32(c1) * b.astype(F32)
    assert t.dtype == F32
    return np.where(t > 0, t, F32(0.0)).astype(F32) if relu else t


# ---- the cases: geometry x mode. Modes 0 and 3 cannot make an output dimension of 1; mode 2 reads its scale from the sizes where given --------
GEOMETRIES = {
    "up_5x7_11x13": (5, 7, 11, 13),          # non-integer upscale, H != W
    "down_9x11_4x5": (9, 11, 4, 5),          # downscale
    "same_7x7": (7, 7, 7, 7),                # identity
    "x2_4x6": (4, 6, 8, 12),                 # x2, even
    "x2_3x5": (3, 5, 6, 10),                 # x2, odd
    "x8_3x5": (3, 5, 24, 40),                # x8
    "row_1x6_3x12": (1, 6, 3, 12),           # an input axis of 1
    "col_6x1_12x3": (6, 1, 12, 3),
    "ties_2x2_3x3": (2, 2, 3, 3),            # nearest with exact .5 ties
}
MODES = (BILINEAR_ALIGN, BILINEAR_NO_ALIGN, RESIZE_CUSTOM, NEAREST_ALIGN)


def geometry_cases(n, c):
    """every geometry x every mode, plus mode 1 to 1 x 1 and mode 2 by scale 2.5 and 0.4 (the zero taps at the right and bottom edge)"""
    out = {}
    for g, (h, w, oh, ow) in GEOMETRIES.items():
        for m in MODES:
            out["%s_m%d" % (g, m)] = case(n, c, h, w, m, oh, ow)
    out["to_1x1_m1"] = case(n, c, 5, 7, BILINEAR_NO_ALIGN, 1, 1)
    out["scale2.5_m2"] = case(n, c, 5, 7, RESIZE_CUSTOM, scale_h=2.5, scale_w=2.5)
    out["scale0.4_m2"] = case(n, c, 9, 11, RESIZE_CUSTOM, scale_h=0.4, scale_w=0.4)
    return out


def make(cs, rng):
    return rng.standard_normal((cs["n"], cs["c"], cs["h"], cs["w"])).astype(F32)


def seed_of(name):
    return int(np.frombuffer(name.encode().ljust(8, b"_")[:8], np.uint32).sum() % (1 << 31))


# the golden fixture's cases (tests/golden/resize_ref.npz, scripts/record_resize_golden.py): every mode on the geometries where modes differ most
GOLDEN_CASES = {}
for _g in ("up_5x7_11x13", "down_9x11_4x5", "x2_3x5", "col_6x1_12x3", "ties_2x2_3x3"):
    for _m in MODES:
        GOLDEN_CASES["%s_m%d" % (_g, _m)] = geometry_cases(2, 3)["%s_m%d" % (_g, _m)]
for _k in ("to_1x1_m1", "scale2.5_m2", "scale0.4_m2"):
    GOLDEN_CASES[_k] = geometry_cases(2, 3)[_k]


# ---- an FPN-style op list: three strided convs, three 1x1 laterals, two top-down nearest x2 + sum merges, a smoothing conv, a bilinear head ----
def fpn_list(n):
    """the layers of the list in order: (kind, name, inputs, params). conv: (w [k, c, ks, ks], bias, stride, pad, relu); resize: a case;
    sum: (c0, c1, relu). Tensors are NCHW-logical here; the executor test stores them NHWC."""
    rng = np.random.default_rng(131072)

    def wb(k, c, ks):
        return (rng.standard_normal((k, c, ks, ks)) * (1.0 / np.sqrt(c * ks * ks))).astype(F32), (rng.standard_normal(k) * 0.1).astype(F32)
    x = rng.standard_normal((n, 3, 32, 32)).astype(F32)
    layers = [
        ("conv", "c1", ["x"], wb(32, 3, 3) + (2, 1, True)),          # 16 x 16
        ("conv", "c2", ["c1"], wb(64, 32, 3) + (2, 1, True)),        # 8 x 8
        ("conv", "c3", ["c2"], wb(64, 64, 3) + (2, 1, True)),        # 4 x 4
        ("conv", "l3", ["c3"], wb(32, 64, 1) + (1, 0, False)),
        ("conv", "l2", ["c2"], wb(32, 64, 1) + (1, 0, False)),
        ("conv", "l1", ["c1"], wb(32, 32, 1) + (1, 0, False)),
        ("resize", "u3", ["l3"], case(n, 32, 4, 4, NEAREST_ALIGN, 8, 8)),
        ("sum", "p2", ["u3", "l2"], (1.0, 1.0, False)),
        ("resize", "u2", ["p2"], case(n, 32, 8, 8, NEAREST_ALIGN, 16, 16)),
        ("sum", "p1", ["l1", "u2"], (1.0, 1.0, False)),              # the resized edge as the SECOND operand
        ("conv", "s1", ["p1"], wb(32, 32, 3) + (1, 1, True)),
        ("resize", "out", ["s1"], case(n, 32, 16, 16, BILINEAR_NO_ALIGN, 32, 32)),
    ]
    return x, layers
