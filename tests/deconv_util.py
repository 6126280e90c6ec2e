"""What the deconv tests share (tests/test_deconv_cpu.py, tests/test_gpu_deconv.py): the cases, the expected values, the single-term probes.

Expected values come from deconv_ref: a float64 numpy SCATTER that restates the col2im rule of include/saber_hip.h -
  input pixel (ih, iw), tap (a, b) lands on output (ih * stride - pad + a * dil, iw * stride - pad + b * dil), summed over the group's
  input channels; OH = (h - 1) * stride + dil * (k - 1) + 1 - 2 * pad -
the opposite loop nest of both kernels (they gather). The compiled reference under oracle/ has no deconv and cannot gain one; the CPU test
ties this rule to torch's conv_transpose2d and to the project's FP32 oracle conv on the zero-inserted input.

Weights are [C, K / group, kh, kw]; tensors here are NCHW-logical numpy arrays."""
import numpy as np

from tests import fp32_probe as FP


def case(n, h, w, c, k, kh, kw=None, stride=(2, 2), pad=(0, 0), dil=(1, 1), group=1):
    return dict(n=n, h=h, w=w, c=c, k=k, kh=kh, kw=kh if kw is None else kw, stride=tuple(stride), pad=tuple(pad), dil=tuple(dil), group=group)


# the smallest shapes at which each mechanism of the bf16-plane kernel can fail (N, H x W, C -> K)
B3_CASES = {
    "k2s2p0": case(2, 3, 5, 32, 16, 2),                               # one tap per phase: the pixel-shuffled 1x1 conv
    "k4s2p1": case(1, 5, 7, 64, 48, 4, pad=(1, 1)),                   # taps leave the image on all four sides, K not a multiple of 64
    "k3s2p1": case(2, 4, 6, 32, 32, 3, pad=(1, 1)),                   # 4 / 2 / 2 / 1 taps per phase, odd outputs
    "k3s2p0": case(2, 4, 6, 32, 32, 3),
    "k4s2p0": case(1, 4, 4, 32, 16, 4),                               # a cell row / column past the image
    "k4s2p3": case(1, 4, 4, 32, 16, 4, pad=(3, 3)),
    "ragged": case(3, 17, 9, 96, 80, 4, pad=(1, 1)),                  # partial cell tiles, three slabs, batch stride, two channel blocks
}
OLD_B3 = tuple(B3_CASES)      # one cell tile along x each (b3_classes): what the seam cases below were added to
# more than one cell tile along x: tile tx takes its left halo from columns of tile tx - 1. (cells h x w; column tiles; what it reaches)
B3_CASES.update({
    "seam_k4p1": case(1, 3, 16, 32, 16, 4, pad=(1, 1)),               # 4 x 17; 2, the last 1 column wide: the k4 halo column read across the seam
    "seam_k2p0": case(2, 2, 17, 32, 16, 2),                           # 2 x 17; 2: no halo, two images
    "seam_k3p1": case(1, 9, 33, 96, 80, 3, pad=(1, 1)),               # 9 x 33; 3: a middle tile, slab 2 lands in LDS buffer 0, two channel blocks
    "seam_k4p2x0": case(2, 9, 20, 64, 144, 4, pad=(2, 0)),            # 8 x 21; 2: q0_h != q0_w, the third channel block has one live tile of four
    "seam_k3p0x2": case(1, 5, 18, 32, 64, 3, pad=(0, 2)),             # 6 x 17; 2: the other pad order, K exactly 64
    "seam_k4p1_twin": case(2, 16, 33, 128, 128, 4, pad=(1, 1)),       # 17 x 34; 3: a scaled twin of the measured k4 p1 rows, four slabs
    "seam_k2p0_twin": case(2, 5, 17, 96, 16, 2),                      # 5 x 17; 2: the measured k2 rows' (k, pad): >= 2 tiles both ways, three slabs
    "seam_k3p1_twin": case(2, 5, 17, 96, 16, 3, pad=(1, 1)),          # 5 x 17; 2: the measured k3 row's (k, pad) likewise
    "seam_k4p1x2_full": case(1, 2, 33, 32, 16, 4, pad=(1, 2)),        # 3 x 32; 2 full column tiles starting at cell q0_w = 1
    "seam_k4p1_probe": case(1, 3, 17, 64, 32, 4, pad=(1, 1)),         # 4 x 18; 2, two slabs: small enough for the single-term probes
    "seam_k3p1_probe": case(1, 2, 17, 64, 32, 3, pad=(1, 1)),         # 2 x 17; 2, two slabs
})
PROBE_CASES = ("k2s2p0", "k4s2p1", "k3s2p1", "seam_k4p1_probe", "seam_k3p1_probe")
# form 0 beyond one grid stride: launch_deconv_direct_f32 caps the grid at 16 384 blocks of 256 lanes, this case has 4 259 840 outputs
STRIDE_CASES = {"two_grid_strides": case(2, 64, 64, 2, 130, 2)}
MAC_BUDGET = 3e8              # multiply-adds of a case's float64 reference (under a second)
# direct kernel only
DIRECT_CASES = {
    "group2": case(2, 4, 5, 8, 6, 3, pad=(1, 1), group=2),
    "depthwise_k4s2p1": case(1, 5, 4, 12, 12, 4, pad=(1, 1), group=12),
    "dil2": case(1, 5, 6, 6, 7, 3, stride=(1, 1), pad=(2, 2), dil=(2, 2)),
    "k2x3_s2x1_p0x1": case(2, 4, 5, 5, 4, 2, 3, stride=(2, 1), pad=(0, 1)),
    "k3s1p1": case(1, 6, 5, 7, 9, 3, stride=(1, 1), pad=(1, 1)),
    "k5s3p1": case(1, 4, 3, 4, 6, 5, stride=(3, 3), pad=(1, 1)),
    "c3k5": case(2, 5, 5, 3, 5, 2),
}
ALL_CASES = dict(B3_CASES, **DIRECT_CASES)


def out_hw(cs):
    return tuple((cs[d] - 1) * cs["stride"][i] + cs["dil"][i] * (cs[kk] - 1) + 1 - 2 * cs["pad"][i] for i, (d, kk) in enumerate((("h", "kh"), ("w", "kw"))))


def macs(cs):
    """multiply-adds of deconv_ref"""
    return cs["n"] * cs["h"] * cs["w"] * cs["c"] * (cs["k"] // cs["group"]) * cs["kh"] * cs["kw"]


def b3_classes(cs):
    """what a bf16-plane launch of the case looks like, computed as launch_deconv_b3_f32 and deconv_b3_f32_kernel do (deconv.hip): the
    first cell q0 = pad div 2 per axis, the cell counts over t = o + pad in [pad, O - 1 + pad], the tiles of TH x 16 cells per form,
    the 32-channel slabs, the 64-channel blocks"""
    (ph, pw), (oh, ow) = cs["pad"], out_hw(cs)
    q0h, q0w = ph // 2, pw // 2
    qh, qw = (oh - 1 + ph) // 2 - q0h + 1, (ow - 1 + pw) // 2 - q0w + 1
    tiles_x = (qw + 15) // 16
    return dict(q0=(q0h, q0w), cells=(qh, qw), tiles_x=tiles_x, tiles_y={1: (qh + 3) // 4, 2: (qh + 1) // 2}, last_cols=qw - 16 * (tiles_x - 1),
                nslab=cs["c"] // 32, ntile=cs["k"] // 16, nky=(cs["k"] + 63) // 64, pads_equal=ph == pw)


def _at_least(v, top=3):
    return min(v, top)


def b3_coverage(cases):
    """the classes a set of bf16-plane cases reaches, as the set of the names below; REQUIRED_CLASSES is what tests/test_deconv_cpu.py asks of
    B3_CASES and of the sweep's draws"""
    got = set()
    for cs in cases:
        cl = b3_classes(cs)
        tx = cl["tiles_x"]
        got.add("tiles_x %d" % _at_least(tx))
        got.add("nslab %d" % _at_least(cl["nslab"]))
        got.add("nky %d" % _at_least(cl["nky"]))
        if cl["last_cols"] in (1, 16):
            got.add("last tile %d" % cl["last_cols"])
        if tx >= 2 and min(cl["tiles_y"].values()) >= 2:
            got.add("tiles both ways")
        if cs["pad"][0] != cs["pad"][1]:
            got.add("pad_h < pad_w" if cs["pad"][0] < cs["pad"][1] else "pad_h > pad_w")
        if tx >= 2:
            got.add("k%d seam" % cs["kh"])
            if cs["n"] > 1:
                got.add("batch seam")
    return got


REQUIRED_CLASSES = {"tiles_x 1", "tiles_x 2", "tiles_x 3", "last tile 1", "last tile 16", "tiles both ways", "nslab 1", "nslab 2", "nslab 3",
                    "nky 1", "nky 2", "nky 3", "pad_h < pad_w", "pad_h > pad_w", "k2 seam", "k3 seam", "k4 seam", "batch seam"}


def make(cs, rng, bias=True):
    x = rng.standard_normal((cs["n"], cs["c"], cs["h"], cs["w"])).astype(np.float32)
    w = (rng.standard_normal((cs["c"], cs["k"] // cs["group"], cs["kh"], cs["kw"])) * 0.3).astype(np.float32)
    b = rng.standard_normal(cs["k"]).astype(np.float32) if bias else None
    return x, w, b


def deconv_ref(x, w, bias, cs, relu=False):
    """float64 scatter: [N, K, OH, OW]"""
    (sh, sw), (ph, pw), (dh, dw), g = cs["stride"], cs["pad"], cs["dil"], cs["group"]
    N, C, H, W = x.shape
    _, Kg, kh, kw = w.shape
    Cg, K = C // g, Kg * g
    oh, ow = out_hw(cs)
    full = np.zeros((N, K, (H - 1) * sh + dh * (kh - 1) + 1, (W - 1) * sw + dw * (kw - 1) + 1), np.float64)
    x64, w64 = x.astype(np.float64), w.astype(np.float64)
    for gi in range(g):
        xs, ws = x64[:, gi * Cg:(gi + 1) * Cg], w64[gi * Cg:(gi + 1) * Cg]
        for a in range(kh):
            for b in range(kw):
                full[:, gi * Kg:(gi + 1) * Kg, a * dh:a * dh + (H - 1) * sh + 1:sh, b * dw:b * dw + (W - 1) * sw + 1:sw] += \
                    np.einsum("nchw,ck->nkhw", xs, ws[:, :, a, b])
    y = full[:, :, ph:ph + oh, pw:pw + ow]
    assert y.shape == (N, K, oh, ow), (y.shape, oh, ow)
    if bias is not None:
        y = y + bias.astype(np.float64)[None, :, None, None]
    return np.maximum(y, 0.0) if relu else y


def as_conv(x, w, cs):
    """the same operator as a stride-1 convolution: (zero-inserted input, OIHW weights flipped and transposed per group, pad, dilation)"""
    (sh, sw), (ph, pw), (dh, dw), g = cs["stride"], cs["pad"], cs["dil"], cs["group"]
    N, C, H, W = x.shape
    _, Kg, kh, kw = w.shape
    Cg = C // g
    xz = np.zeros((N, C, (H - 1) * sh + 1, (W - 1) * sw + 1), x.dtype)
    xz[:, :, ::sh, ::sw] = x
    wc = np.concatenate([w[gi * Cg:(gi + 1) * Cg, :, ::-1, ::-1].transpose(1, 0, 2, 3) for gi in range(g)], axis=0)      # [K, Cg, kh, kw]
    return xz, np.ascontiguousarray(wc), (dh * (kh - 1) - ph, dw * (kw - 1) - pw), (dh, dw)


def fp32_close(got_nchw, want_nchw, what, rtol=1e-4):
    """the project's two FP32 criteria (_fp32_close of tests/test_gpu_dw.py): the largest error relative to the largest value, and every
    element's error relative to |value| + mean |value|"""
    want = np.asarray(want_nchw, np.float64)
    d = np.abs(np.asarray(got_nchw, np.float64) - want)
    e_max = float(d.max() / max(np.abs(want).max(), 1e-30))
    e_el = float((d / (np.abs(want) + np.abs(want).mean() + 1e-30)).max())
    assert e_max <= rtol and e_el <= rtol, (what, e_max, e_el)
    return e_max, e_el


# ---- the packed fragment stream ([phase][tap][32-deep slab][16-channel tile][plane][lane] x 8 bf16, anakin_amd/csrc/deconv.hip) -------------
def stream_taps(k):
    """the stream's [phase][tap] order: (phase, a, b) with phase = 2 (a mod 2) + (b mod 2), taps row-major inside a phase"""
    out = []
    for rh in range(2):
        for rw in range(2):
            out += [(2 * rh + rw, a, b) for a in range(rh, k, 2) for b in range(rw, k, 2)]
    return out


def phase_taps(k, pad, o):
    """the taps (along one axis) that reach output coordinate o of a stride-2 deconv, with the input coordinate each reads: phase
    r = (o + pad) mod 2, cell q = (o + pad) div 2, tap a = r + 2 j on input q - j"""
    t = o + pad
    return [(a, t // 2 - (a - t % 2) // 2) for a in range(t % 2, k, 2)]


# ---- single-term probes ---------------------------------------------------------------------------------------------------------------
class DeconvProbe(FP.Probe):
    """fp32_probe.Probe for a deconv: x [N, C, H, W], w [C, K, kh, kw] (group 1), out_idx flat in [N, K, OH, OW]. Everything that reads a
    probe (emulate, failures) finds the same fields."""

    def __init__(self, cs, x, w, bias, out_idx, x_idx, w_idx, relu=False):
        self.cs, self.x, self.w, self.bias, self.relu, self.pool = cs, x, w, bias, relu, None
        self.geo = (cs["n"], cs["h"], cs["w"], cs["c"], cs["k"], cs["kh"], cs["pad"][0], cs["stride"][0], 1)
        self.out_idx, self.x_idx, self.w_idx, self.w_exact = out_idx, x_idx, w_idx, w
        self.conv_shape = (cs["n"], cs["k"]) + out_hw(cs)
        assert len(np.unique(out_idx)) == len(out_idx), "two terms in one output"
        assert not (relu and bias is not None)
        self.term = x.astype(np.float64).ravel()[x_idx] * w.astype(np.float64).ravel()[w_idx]
        e = np.zeros(self.conv_shape, np.float64)
        e.ravel()[out_idx] = self.term
        mag = np.abs(e)
        if bias is not None:
            b = bias.astype(np.float64)[None, :, None, None]
            e, mag = e + b, mag + np.abs(b)
        if relu:
            e = np.maximum(e, 0.0)
            mag = e
        self.exact, self.bound = e, FP.BOUND_U * FP.U * mag

    def check(self, got, what=""):
        bad = self.failures(got)
        if len(bad):
            i = tuple(int(v) for v in bad[0])
            raise AssertionError("%s: %d of %d outputs outside %g u, first out[n, k, y, x] = %s: got %.9g exact %.9g (case %s)" %
                                 (what, len(bad), self.exact.size, FP.BOUND_U, i, float(np.asarray(got)[i]), float(self.exact[i]), self.cs))


def _terms(cs, n_i, ci, py, px, kmask=None):
    """every (output, input, weight) index triple of the input elements x[n_i, ci, py, px] of a dense-weight probe"""
    (sh, sw), (ph, pw), (dh, dw) = cs["stride"], cs["pad"], cs["dil"]
    C, K, H, W, kh, kw = cs["c"], cs["k"], cs["h"], cs["w"], cs["kh"], cs["kw"]
    oh, ow = out_hw(cs)
    oi, xi, wi = [], [], []
    karr = np.arange(K)[None, :]
    for a in range(kh):
        oy = py * sh - ph + a * dh
        for b in range(kw):
            ox = px * sw - pw + b * dw
            v = (oy >= 0) & (oy < oh) & (ox >= 0) & (ox < ow)
            if not v.any():
                continue
            oi.append((((n_i[v][:, None] * K + karr) * oh + oy[v][:, None]) * ow + ox[v][:, None]).ravel())
            xi.append(np.broadcast_to((((n_i[v] * C + ci[v]) * H + py[v]) * W + px[v])[:, None], (int(v.sum()), K)).ravel())
            wi.append((((ci[v][:, None] * K + karr) * kh + a) * kw + b).ravel())
    return np.concatenate(oi), np.concatenate(xi), np.concatenate(wi)


def weight_probes(cs, rng, bias=False, max_passes=4000):
    """Dense weights, input zero except on a pixel lattice of pitch ceil(k / stride) - the footprints (k x k outputs, stride apart) of two
    lattice pixels never overlap - with one non-zero channel per lattice pixel; passes until every weight element that reaches an output was
    the factor of a checked output. Returns (passes, weight coverage [C, K, kh, kw], reachable weights)."""
    C, K, H, W, kh, kw, N = cs["c"], cs["k"], cs["h"], cs["w"], cs["kh"], cs["kw"], cs["n"]
    S = [-(-cs[kk] // cs["stride"][i]) for i, kk in enumerate(("kh", "kw"))]
    w = FP.rand_f32(rng, (C, K, kh, kw))
    b = FP.rand_f32(rng, (K,)) if bias else None
    # a tap no input pixel brings inside the output (k4 s2 p3 on a small image) cannot be probed: not part of "every weight"
    every = np.ones(N * H * W, int)
    n_a, y_a, x_a = [v.ravel() for v in np.meshgrid(np.arange(N), np.arange(H), np.arange(W), indexing="ij")]
    reach = np.zeros((C, K, kh, kw), bool)
    _, _, wi = _terms(cs, n_a, np.zeros_like(every), y_a, x_a)
    tap_ok = np.zeros((kh, kw), bool)
    tap_ok.ravel()[np.unique(wi % (kh * kw))] = True
    reach[:] = tap_ok[None, None]
    cov = np.zeros((C, K, kh, kw), bool)
    passes, q = [], 0
    origins = [(a, c) for a in range(S[0]) for c in range(S[1])]
    for t in range(max_passes):
        if (cov | ~reach).all():
            break
        a0, b0 = origins[t % len(origins)]
        ys, xs = np.arange(a0, H, S[0]), np.arange(b0, W, S[1])
        if len(ys) == 0 or len(xs) == 0:
            continue
        n_i, py, px = [v.ravel() for v in np.meshgrid(np.arange(N), ys, xs, indexing="ij")]
        T = len(n_i)
        ch = (q + np.arange(T)) % C
        q += T + (1 if T % C == 0 else 0)
        x = np.zeros((N, C, H, W), np.float32)
        x[n_i, ch, py, px] = FP.rand_f32(rng, (T,))
        p = DeconvProbe(cs, x, w, b, *_terms(cs, n_i, ch, py, px))
        cov.ravel()[p.w_idx[p.term != 0.0]] = True
        passes.append(p)
    else:
        raise AssertionError("deconv weight probes: coverage not full after %d passes (%s)" % (max_passes, cs))
    return passes, cov, reach


def activation_probes(cs, rng, bias=False, max_sets=4000):
    """Dense input, one non-zero weight per output channel at a (channel, tap) position that walks over all C * kh * kw positions; sets
    until every position was used and every input element that reaches an output was the factor of a checked output. Returns (passes, input
    coverage [N, C, H, W], position coverage [C, kh, kw], reachable inputs)."""
    (sh, sw), (ph, pw), (dh, dw) = cs["stride"], cs["pad"], cs["dil"]
    C, K, H, W, kh, kw, N = cs["c"], cs["k"], cs["h"], cs["w"], cs["kh"], cs["kw"], cs["n"]
    oh, ow = out_hw(cs)
    npos = C * kh * kw
    xcov, poscov = np.zeros((N, C, H, W), bool), np.zeros((C, kh, kw), bool)
    iy, ix = np.arange(H), np.arange(W)
    ry = np.zeros(H, bool)
    rx = np.zeros(W, bool)
    for a in range(kh):
        ry |= (iy * sh - ph + a * dh >= 0) & (iy * sh - ph + a * dh < oh)
    for b in range(kw):
        rx |= (ix * sw - pw + b * dw >= 0) & (ix * sw - pw + b * dw < ow)
    xread = np.broadcast_to((ry[:, None] & rx[None, :])[None, None], (N, C, H, W))
    passes, s = [], 0
    while not (s * K >= npos and (xcov | ~xread).all()):
        if s >= max_sets:
            raise AssertionError("deconv activation probes: coverage not full after %d weight sets (%s)" % (max_sets, cs))
        pos = (s * K + np.arange(K)) % npos
        tap, c_k = pos // C, pos % C
        a_k, b_k = tap // kw, tap % kw
        w = np.zeros((C, K, kh, kw), np.float32)
        w[c_k, np.arange(K), a_k, b_k] = FP.rand_f32(rng, (K,))
        b = FP.rand_f32(rng, (K,)) if bias else None
        oy = iy[None, :] * sh - ph + a_k[:, None] * dh          # [K, H]
        ox = ix[None, :] * sw - pw + b_k[:, None] * dw          # [K, W]
        valid = ((oy >= 0) & (oy < oh))[:, :, None] & ((ox >= 0) & (ox < ow))[:, None, :]
        kk, vy, vx = np.nonzero(valid)
        nn = np.arange(N)[:, None]
        out_idx = (((nn * K + kk[None]) * oh + oy[kk, vy][None]) * ow + ox[kk, vx][None]).ravel()
        x_idx = (((nn * C + c_k[kk][None]) * H + vy[None]) * W + vx[None]).ravel()
        w_idx = np.broadcast_to(np.ravel_multi_index((c_k[kk], kk, a_k[kk], b_k[kk]), w.shape)[None], (N, len(kk))).ravel()
        x = FP.rand_f32(rng, (N, C, H, W))
        p = DeconvProbe(cs, x, w, b, out_idx, x_idx, w_idx)
        xcov.ravel()[p.x_idx[p.term != 0.0]] = True
        poscov[c_k, a_k, b_k] = True
        passes.append(p)
        s += 1
    return passes, xcov, poscov, xread


def build_probes(name):
    """the probes of a case, the same in the CPU test and the GPU test: {"weight": (...), "activation": (...)}; the first case also runs
    with a bias"""
    cs = B3_CASES[name]
    rng = np.random.default_rng(FP._seed("deconv/" + name))
    bias = name == PROBE_CASES[0]
    return {"weight": weight_probes(cs, rng, bias=bias), "activation": activation_probes(cs, rng, bias=bias)}


def wrong_phase(p):
    """the probe a kernel sees that assigns taps a = 0 and a = 1 to each other's phase (the fragment stream's first two tap rows swapped)"""
    w = p.w.copy()
    w[:, :, [0, 1]] = w[:, :, [1, 0]]
    q = DeconvProbe(p.cs, p.x, w, p.bias, p.out_idx, p.x_idx, p.w_idx)
    return q


# ---- random-geometry sweep: the class is drawn first (enumerated from the draw's index), then a shape inside it ----------------------------
SWEEP_SEEDS = (0, 1, 2)
SWEEP_DIRECT, SWEEP_B3 = 8, 9      # draws per seed: 24 direct launches, 27 bf16-plane cases x 3 forms


def _pick(rng, seq):
    return seq[int(rng.integers(len(seq)))]


def _direct_draw(rng, i, seed):
    """form 0 only. i enumerates: the layout pair (i mod 4), the group class (1 | depthwise | a proper divisor of gcd(C, K)), whether the
    strides differ, whether a dilation is 2; the rest is drawn. Ragged C and K, kh != kw in 1 .. 5, stride 1 .. 3, pad 0 .. dil (k - 1)."""
    j = i + seed
    while True:
        gclass = j % 3
        if gclass == 0:
            g, c, k = 1, _pick(rng, (1, 3, 5, 7, 9, 11)), _pick(rng, (1, 3, 5, 7, 9, 13))
        elif gclass == 1:
            g = _pick(rng, (3, 5, 7, 12))
            c = k = g
        else:
            g = _pick(rng, (2, 3, 5))
            c, k = g * _pick(rng, (1, 3, 5)), g * _pick(rng, (3, 5, 7))
        kh = int(rng.integers(1, 6))
        kw = _pick(rng, [v for v in range(1, 6) if v != kh])
        sh = int(rng.integers(1, 4))
        sw = _pick(rng, [v for v in range(1, 4) if v != sh]) if (j // 3) % 2 == 0 else int(rng.integers(1, 4))
        dh, dw = (2, int(rng.integers(1, 3))) if (j // 2) % 2 == 0 else (int(rng.integers(1, 3)), int(rng.integers(1, 3)))
        if (j // 2) % 4 == 2:
            dh, dw = dw, dh
        cs = case(int(rng.integers(1, 4)), int(rng.integers(1, 10)), int(rng.integers(1, 10)), c, k, kh, kw, stride=(sh, sw),
                  pad=(int(rng.integers(0, dh * (kh - 1) + 1)), int(rng.integers(0, dw * (kw - 1) + 1))), dil=(dh, dw), group=g)
        if min(out_hw(cs)) >= 1 and macs(cs) <= MAC_BUDGET:      # an empty output is redrawn inside the same class, never skipped
            return dict(cs=cs, in_nchw=bool(i & 1), out_nchw=bool(i & 2), bias=bool(rng.integers(2)), relu=bool(rng.integers(2)))


def _b3_draw(rng, i, seed):
    """forms 0, 1, 2. (i, seed) enumerates every (k, column-tile class, row-tile class) of {2, 3, 4} x {1, 2, 3} x {1, 2, >= 3} once over the
    three seeds - row tiles counted for the 4 x 16 form - and walks the slab count, the channel-block count and the last tile's width
    (any | 1 | 16 columns); pads, the shape inside the class, the batch, bias and relu are drawn."""
    txc, tyc = divmod(i, 3)
    k = (2, 3, 4)[(i + seed) % 3]
    c = (32, 64, 96, 128)[(i + seed) % 4]
    kout = _pick(rng, ((16, 32, 48, 64), (80, 96, 112, 128), (144, 160))[(i // 3 + seed) % 3])
    last = (None, 1, 16)[(i + 2 * seed) % 3]
    while True:
        pad = (int(rng.integers(0, k)), int(rng.integers(0, k)))
        hs, ws = [], []
        for v in range(1, 64):
            cs = case(1, v, v, c, kout, k, pad=pad)
            if min(out_hw(cs)) < 1:
                continue
            cl = b3_classes(cs)
            if _at_least(cl["tiles_y"][1]) == tyc + 1 and cl["tiles_y"][1] <= 3:
                hs.append(v)
            if cl["tiles_x"] == txc + 1 and (last is None or cl["last_cols"] == last):
                ws.append(v)
        if not hs or not ws:
            continue
        cs = case(int(rng.integers(1, 4)), _pick(rng, hs), _pick(rng, ws), c, kout, k, pad=pad)
        if macs(cs) > MAC_BUDGET:
            cs["n"] = 1
        if macs(cs) <= MAC_BUDGET:
            return dict(cs=cs, bias=bool(rng.integers(2)), relu=bool(rng.integers(2)))


def sweep_draws(seed):
    """{"direct": [draw], "b3": [draw]}: the same draws in the CPU test (coverage, the torch tie) and in the GPU test"""
    rng = np.random.default_rng([20260, seed])
    return {"direct": [_direct_draw(rng, i, seed) for i in range(SWEEP_DIRECT)], "b3": [_b3_draw(rng, i, seed) for i in range(SWEEP_B3)]}
