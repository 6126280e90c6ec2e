"""Per-axis convolution and pooling geometry (kh != kw, pad_h != pad_w, stride_h != stride_w, dil_h != dil_w): the case tables, the data
and the generators that tests/test_asym_cpu.py and tests/test_gpu_asym.py share. TEST INFRASTRUCTURE ONLY.

Every other suite hands both axes of a pair the same value, so a kernel, weight packer or eligibility rule that reads pad_h where it means
pad_w is invisible to it. Every case here has H != W and at least one pair whose two values differ; tests/test_asym_cpu.py proves on the
oracle that each such swap changes the output of each case."""
import zlib

import numpy as np

from oracle import oracle as O

F32, S8, U8 = O.F32, O.S8, O.U8

# name -> (N, H, W, C, K, (kh, kw), (pad_h, pad_w), (stride_h, stride_w), (dil_h, dil_w), group): the smallest shape that reaches each family
ASYM_CONV_CASES = {
    "k1x7":       (1, 9, 13, 64, 32, (1, 7), (0, 3), (1, 1), (1, 1), 1),       # implicit GEMM, taps along W only
    "k7x1":       (1, 13, 9, 64, 32, (7, 1), (3, 0), (1, 1), (1, 1), 1),       # ... along H only
    "p01":        (2, 10, 11, 64, 64, (3, 3), (0, 1), (1, 1), (1, 1), 1),      # implicit GEMM, halo kernels
    "p10":        (2, 10, 11, 64, 64, (3, 3), (1, 0), (1, 1), (1, 1), 1),
    "img_p01":    (1, 7, 6, 512, 32, (3, 3), (0, 1), (1, 1), (1, 1), 1),       # image-resident 3x3 (variant 9)
    "img_p10":    (1, 7, 6, 512, 32, (3, 3), (1, 0), (1, 1), (1, 1), 1),
    "s21":        (1, 12, 15, 64, 32, (3, 3), (1, 1), (2, 1), (1, 1), 1),
    "s12":        (1, 12, 15, 64, 32, (3, 3), (1, 1), (1, 2), (1, 1), 1),
    "d21":        (1, 12, 15, 16, 16, (3, 3), (2, 1), (1, 1), (2, 1), 1),
    "d12":        (1, 12, 15, 16, 16, (3, 3), (1, 2), (1, 1), (1, 2), 1),
    "c3_3x5":     (1, 11, 14, 3, 16, (3, 5), (1, 2), (2, 1), (1, 1), 1),       # the NHWC4 first-layer path: kw padded to 8
    "c4_5x3":     (1, 11, 14, 4, 16, (5, 3), (2, 1), (1, 2), (1, 1), 1),       # ... kw padded to 4
    "stem_p32":   (1, 30, 27, 3, 64, (7, 7), (3, 2), (2, 2), (1, 1), 1),       # stem kernel
    "stem_p23":   (1, 30, 27, 3, 64, (7, 7), (2, 3), (2, 2), (1, 1), 1),
    "pw_p10_s12": (1, 8, 9, 64, 64, (1, 1), (1, 0), (1, 2), (1, 1), 1),        # 1x1 with a padded, strided axis each
    "g4_3x1":     (1, 9, 10, 32, 32, (3, 1), (1, 0), (1, 1), (1, 1), 4),       # direct kernels
    "dw_p10":     (1, 9, 10, 64, 64, (3, 3), (1, 0), (1, 1), (1, 1), 64),      # depthwise: variant 16 must refuse
    "dw_s21":     (1, 9, 10, 64, 64, (3, 3), (1, 1), (2, 1), (1, 1), 64),
    "g16_s12":    (1, 9, 10, 64, 64, (3, 3), (1, 1), (1, 2), (1, 1), 16),      # Cg = 4 grouped: variant 17 must refuse
    "n3_k34_3x1": (3, 7, 10, 32, 34, (3, 1), (1, 0), (1, 1), (1, 1), 1),       # three images, K % 16 != 0: the generic epilogue
    "c256_3x1":   (1, 6, 9, 256, 64, (3, 1), (1, 0), (2, 1), (1, 1), 1),       # 24 reduction steps of 32: every FP32 split-K factor
    "c32_3x5":    (1, 9, 12, 32, 24, (3, 5), (1, 2), (1, 1), (1, 1), 1),       # a 2-D non-square tap walk on the generic implicit GEMM and,
                                                                               # C % 8 == 0, on the bf16-plane tiles, 8-wave forms and split-K
}
PAIRS = ("kernel", "pad", "stride", "dil")      # tuple index 5 .. 8


def out_hw(case):
    N, H, W, C, K, k, pad, stride, dil, g = case
    return O.conv_out_hw(H, W, k[0], k[1], pad, stride, dil)


def differing_pairs(case):
    return [PAIRS[i] for i in range(4) if case[5 + i][0] != case[5 + i][1]]


def transposed(case):
    """the same convolution on the H <-> W transposed image: every pair swapped"""
    N, H, W, C, K, k, pad, stride, dil, g = case
    return (N, W, H, C, K) + tuple(p[::-1] for p in (k, pad, stride, dil)) + (g,)


for _n, _c in ASYM_CONV_CASES.items():
    assert _c[1] != _c[2] and differing_pairs(_c) and min(out_hw(_c)) >= 1 and _c[3] % _c[9] == 0 and _c[4] % _c[9] == 0, _n


def seed_of(name, salt=0):
    return (zlib.crc32(name.encode()) + 7919 * salt) & 0x7fffffff


def rand8(rng, shape, dt):
    return rng.integers(0, 256, shape).astype(np.uint8) if dt == U8 else rng.integers(-128, 128, shape).astype(np.int8)


class I8Data:
    """x NHWC s8 / u8, f32 weights and their quantisation, bias, scales of one INT8 case; .want is the oracle's output (computed on demand)"""

    def __init__(self, case, idt, odt, relu, bias=True, seed=0):
        N, H, W, C, K, k, pad, stride, dil, g = case
        rng = np.random.default_rng(seed)
        self.case, self.idt, self.odt, self.relu = case, idt, odt, int(relu)
        self.x = rand8(rng, (N, H, W, C), idt)
        self.w = (rng.standard_normal((K, C // g, k[0], k[1])) * np.sqrt(2.0 / ((C // g) * k[0] * k[1]))).astype(np.float32)
        self.b = (rng.standard_normal(K) * 0.5).astype(np.float32) if bias else None
        # (a u8 image has a mean: its outputs spread twice as wide; these scales leave a few per cent of an 8-bit output on the rails)
        self.in_scale, self.out_scale = 0.017, (0.041 if idt == S8 else 0.09)
        self.ws = O.weight_scales(self.w)
        self.wq = O.quant_weights(self.w, self.ws)
        self._want = None

    def oracle(self, x=None, wq=None, pad=None, stride=None, dil=None, odt=None):
        """the oracle's convolution of this data, any of the operands or pairs replaced"""
        c = self.case
        odt = self.odt if odt is None else odt
        bp, sc = O.conv_i8_prepare(self.ws, self.b, self.in_scale, self.out_scale, self.idt, odt)
        return O.conv_i8(self.x if x is None else x, self.wq if wq is None else wq, bp, sc, odt, self.relu, pad or c[6], stride or c[7],
                         dil or c[8], group=c[9])

    @property
    def want(self):
        if self._want is None:
            self._want = self.oracle()
        return self._want


class F32Data:
    """x NCHW f32, weights, bias of one FP32 case; .want is the oracle's NCHW output with relu"""

    def __init__(self, case, seed=0, relu=True):
        N, H, W, C, K, k, pad, stride, dil, g = case
        rng = np.random.default_rng(seed)
        self.case, self.relu = case, relu
        self.x = (rng.random((N, C, H, W)) * 3.0 - 1.0).astype(np.float32)
        self.w = (rng.standard_normal((K, C // g, k[0], k[1])) * np.sqrt(2.0 / ((C // g) * k[0] * k[1]))).astype(np.float32)
        self.b = (rng.standard_normal(K) * 0.5).astype(np.float32)
        self._want = None

    def oracle(self, x=None, w=None, pad=None, stride=None, dil=None):
        c = self.case
        return O.conv_f32_nchw(self.x if x is None else x, self.w if w is None else w, self.b, self.relu, pad or c[6], stride or c[7],
                               dil or c[8], group=c[9])

    @property
    def want(self):
        if self._want is None:
            self._want = self.oracle()
        return self._want


def swapped_weights(w, how):
    if how == "transpose":
        return np.ascontiguousarray(w.transpose(0, 1, 3, 2))
    if how == "reinterpret":
        K, Cg, kh, kw = w.shape
        return np.ascontiguousarray(w.reshape(K, Cg, kw, kh).transpose(0, 1, 3, 2))
    return w


def swap_situations(case):
    """[(label, weights, pad, stride, dil)]: what a kernel would compute that confuses the two axes of ONE pair that differs - the pair
    swapped, or the value of one axis used for both. For the kernel pair, weights is "transpose" (a kw x kh kernel: the taps [i][j] read as
    [j][i]) or "reinterpret" (the kh x kw kernel whose taps were packed with the other axis's pitch: i * kh + j for i * kw + j)."""
    N, H, W, C, K, k, pad, stride, dil, g = case
    out = []
    if k[0] != k[1]:
        out.append(("weights transposed", "transpose", pad, stride, dil))
        if min(k) > 1:
            out.append(("taps packed with the other pitch", "reinterpret", pad, stride, dil))
    for name, idx in (("pad", 6), ("stride", 7), ("dil", 8)):
        a, b = case[idx]
        if a == b:
            continue
        for label, v in (("%s swapped" % name, (b, a)), ("%s_h for both" % name, (a, a)), ("%s_w for both" % name, (b, b))):
            p = {6: pad, 7: stride, 8: dil}
            p[idx] = v
            out.append((label, None, p[6], p[7], p[8]))
    return out


def situation_out_hw(case, how, pad, stride, dil):
    """output dims of `case` in a swap situation, or None where the kernel's extent exceeds the padded image (no output; Python's floor
    and C's truncating division disagree on a negative numerator, so such a geometry must never reach the oracle)"""
    N, H, W, C, K, k, _, _, _, g = case
    k = k[::-1] if how == "transpose" else k
    num = [(H, W)[a] + 2 * pad[a] - (dil[a] * (k[a] - 1) + 1) for a in range(2)]
    if min(num) < 0:
        return None
    return tuple(num[a] // stride[a] + 1 for a in range(2))


def random_asym_geometry(rng, int8):
    """tests/test_gpu_parity.py:_random_conv_geometry with the two values of every pair drawn independently: kh, kw in {1, 3, 5, 7}, stride
    1 | 2 and dilation 1 | 2 (for more than one tap) per axis, pad 0 | 1 | same-size per axis. Redrawn until the output is not empty and at
    least one pair differs. Returns (N, H, W, C, K, (kh, kw), pad, stride, dil, 1)."""
    while True:
        k = tuple(int(rng.choice([1, 1, 3, 3, 3, 5, 7])) for _ in range(2))
        stride = tuple(int(rng.choice([1, 1, 1, 2])) for _ in range(2))
        dil = tuple(int(rng.choice([1, 1, 1, 2])) if k[a] > 1 else 1 for a in range(2))
        pad = tuple(int(rng.choice([0, (dil[a] * (k[a] - 1)) // 2, (dil[a] * (k[a] - 1)) // 2, 1])) for a in range(2))
        C = int(rng.choice([3, 4, 16, 32, 48, 64, 96, 128, 256, 512]) if int8 else rng.choice([3, 4, 8, 16, 32, 64, 96, 128, 256]))
        K = int(rng.choice([8, 10, 16, 24, 34, 40, 64, 72, 128, 200, 256]))
        N = int(rng.choice([1, 1, 2, 3, 8]))
        lo = [dil[a] * (k[a] - 1) + 1 - 2 * pad[a] for a in range(2)]
        H = int(rng.integers(max(lo[0], 1), 30))
        W = int(rng.integers(max(lo[1], 1), 34))
        if C >= 256 and max(k) >= 5:      # (the cost of the oracle, as in the square draw: the larger tap count drops to 3)
            k = tuple(min(v, 3) for v in k)
            dil = tuple(dil[a] if k[a] > 1 else 1 for a in range(2))
            pad = tuple(min(pad[a], (dil[a] * (k[a] - 1)) // 2) for a in range(2))
        case = (N, H, W, C, K, k, pad, stride, dil, 1)
        oh, ow = out_hw(case)
        if oh >= 1 and ow >= 1 and differing_pairs(case):
            return case


# ---- pooling ------------------------------------------------------------------------------------------------------------------------------
# name -> (N, H, W, C, (win_h, win_w), (stride_h, stride_w), (pad_h, pad_w)); pad < window per axis; every case runs with the three pooling
# types in ceil and in floor mode
ASYM_POOL_CASES = {
    "w23_s21_p01_c3":   (1, 9, 12, 3, (2, 3), (2, 1), (0, 1)),
    "w32_s12_p10_c10":  (2, 11, 8, 10, (3, 2), (1, 2), (1, 0)),
    "w13_s12_p01_c16":  (1, 7, 10, 16, (1, 3), (1, 2), (0, 1)),       # a 1 x k window with stride (1, s)
    "w52_s31_p20_c64":  (1, 10, 7, 64, (5, 2), (3, 1), (2, 0)),
    "w32_s21_p00_c16":  (1, 8, 9, 16, (3, 2), (2, 1), (0, 0)),        # ceil mode: the last window hangs over the far edge of H only
    "w32_s21_p10_c10":  (1, 8, 9, 10, (3, 2), (2, 1), (1, 0)),        # ... and ends past H + pad_h: the averaging divisor clips bh, not bw
    "w23_s12_p01_c64":  (2, 6, 8, 64, (2, 3), (1, 2), (0, 1)),        # the mirror: bw clips, bh does not
    "w13_s31_p01_c4":   (1, 9, 7, 4, (1, 3), (3, 1), (0, 1)),         # stride_h > win_h on the unpadded axis while the other is padded: the
                                                                      # reference drops the window that starts past the image on BOTH axes
}
POOL_TYPES = (0, 1, 2)      # max, average including padding, average excluding padding


def pool_out_hw(case, floor_mode):
    """Pooling<>::compute_output_shape (saber/funcs/pooling.h:92-125) written out: ceil or floor, then - when EITHER pad is non-zero - the
    last window of each axis is dropped if it starts at or past in + pad"""
    N, H, W, C, win, stride, pad = case
    out = []
    for a, inp in enumerate((H, W)):
        q = np.float32(inp + 2 * pad[a] - win[a]) / np.float32(stride[a])
        o = (max(int(q), 0) if floor_mode else int(np.ceil(q))) + 1
        if (pad[0] or pad[1]) and (o - 1) * stride[a] >= inp + pad[a]:
            o -= 1
        out.append(o)
    return tuple(out)


def pool_reference(x, case, ptype, floor_mode, f32):
    """Pooling over an NHWC integer (f32 False) or NCHW float (f32 True) tensor in float64 / exact integers, per-axis slices written out.
    Integer: saber_pooling.cpp:589-654 - max, or the int32 sum times float32(1 / divisor) rounded to nearest even and saturated, divisor
    kh * kw (including padding) or the in-image count. Float: saber_pooling.cpp:385-500 - an empty window gives 0 (max) or 0 / divisor;
    the including-padding divisor is bh * bw, each side clipped at in + pad when the window reaches the image's far edge."""
    N, H, W, C, win, stride, pad = case
    oh, ow = pool_out_hw(case, floor_mode)
    xs = x if not f32 else x.transpose(0, 2, 3, 1)
    out = np.zeros((N, oh, ow, C), np.float64)
    for i in range(oh):
        hs0 = i * stride[0] - pad[0]
        hs, he = max(hs0, 0), min(hs0 + win[0], H)
        for j in range(ow):
            ws0 = j * stride[1] - pad[1]
            ws, we = max(ws0, 0), min(ws0 + win[1], W)
            patch = xs[:, hs:he, ws:we, :].astype(np.float64).reshape(N, -1, C)
            empty = patch.shape[1] == 0
            if ptype == 0:
                out[:, i, j, :] = 0.0 if empty else patch.max(axis=1)
                continue
            s = patch.sum(axis=1)
            if ptype == 2:
                div = (he - hs) * (we - ws)
            elif not f32:
                div = win[0] * win[1]
            else:
                bh, bw = win[0], win[1]
                if we == W:
                    bw = min(ws + win[1], W + pad[1]) - ws
                if he == H:
                    bh = min(hs + win[0], H + pad[0]) - hs
                div = bh * bw
            if f32:
                with np.errstate(divide="ignore", invalid="ignore"):
                    out[:, i, j, :] = s / np.float64(div)
            else:
                out[:, i, j, :] = (s.astype(np.float32) * (np.float32(1.0) / np.float32(div))).astype(np.float64)
    return out if not f32 else out.transpose(0, 3, 1, 2)


# ---- kernel selection (host side: create -> set_tile -> algo needs no device) -------------------------------------------------------------
DW_GROUP_CODES = [(16 << 16) | v for v in range(4)] + [(17 << 16) | v for v in range(3)]      # variants 16 / 17: direct kernel and forms


# every kernel-selection code the library might accept for a conv (tile | stage depth << 8 | variant << 16): the lists of
# tests/test_gpu_parity.py (_I8_CODES, _F32_CODES), restated here so that the host-side tests need neither torch nor a gpu-marked module;
# tests/test_gpu_asym.py asserts that the two spellings agree
I8_CODES = [t | (ks << 8) | (v << 16) for v in (1, 2, 3, 4) for t in range(6) for ks in (1, 2, 4)] + \
           [t | (ks << 8) | (v << 16) for v in (5, 6) for t in range(3) for ks in (1, 2, 4)] + [7 << 16, 8 << 16, 12 << 16] + \
           [rb | ((ib | nw) << 8) | (9 << 16) for rb in (1, 2, 4, 7) for ib in (1, 2) for nw in (0, 0x80)]
F32_CODES = [t | ((ks | (sh << 4)) << 8) | (11 << 16) for t in range(10) for ks in (1, 2) for sh in (0, 1, 2, 3)] + \
            [v | (13 << 16) for v in range(1, 9)] + [v | (14 << 16) for v in range(0, 5)] + \
            [t | (ks << 8) | (v << 16) for v in (1, 2) for t in range(6) for ks in (1, 2, 4)]


def selection_codes(int8):
    """the list above for the precision, plus variants 16 / 17"""
    return (I8_CODES if int8 else F32_CODES) + DW_GROUP_CODES


def create_conv(lib, L, case, int8, in_dt=None, out_dt=None, layout=None):
    """a conv handle for `case` from the descriptor alone (no weights): 8-bit NHWC for INT8, f32 NHWC (or `layout`) for FP32"""
    import ctypes as C
    N, H, W, Cc, K, k, pad, stride, dil, g = case
    d = L.ConvDesc()
    d.n, d.h, d.w, d.c, d.k, d.kh, d.kw = N, H, W, Cc, K, k[0], k[1]
    d.pad_h, d.pad_w = pad
    d.stride_h, d.stride_w = stride
    d.dil_h, d.dil_w = dil
    d.group = g
    d.in_dtype = (L.S8 if int8 else L.F32) if in_dt is None else in_dt
    d.out_dtype = (L.S8 if int8 else L.F32) if out_dt is None else out_dt
    d.in_layout = d.out_layout = L.NHWC if layout is None else layout
    d.int8_weights = 1 if int8 else 0
    d.sum_scale = 1.0
    h = C.c_void_p()
    assert lib.saber_hip_conv2d_create(C.byref(d), C.byref(h)) == 0, lib.saber_hip_last_error()
    return h


def accepted_forms(lib, h, codes):
    """[(code, algo name)]: the selection the op starts with, then every code of `codes` that set_tile accepts, one per kernel name; a
    refused code must leave the selection and the name as they were. The op's own selection is restored."""
    first = (lib.saber_hip_conv2d_get_tile(h), lib.saber_hip_conv2d_algo(h).decode())
    forms, seen = [first], {first[1]}
    for code in codes:
        before = (lib.saber_hip_conv2d_get_tile(h), lib.saber_hip_conv2d_algo(h).decode())
        rc = lib.saber_hip_conv2d_set_tile(h, code)
        name = lib.saber_hip_conv2d_algo(h).decode()
        if rc != 0:
            assert (lib.saber_hip_conv2d_get_tile(h), name) == before, ("a refused code changed the selection", hex(code), before, name)
            continue
        if name not in seen:
            seen.add(name)
            forms.append((code, name))
    assert lib.saber_hip_conv2d_set_tile(h, first[0]) == 0 and lib.saber_hip_conv2d_algo(h).decode() == first[1], first
    return forms
