"""Single-term probes for the FP32 kernels that compute on three bf16 planes (x = h + m + l, six plane products per term).

A dense reduction averages a missing plane or plane product away; one term per output does not: every output of a probe is
x * w for ONE known (input element, weight element) pair, or exactly zero, so a kernel that loses the low plane of one operand, skips one
of the six products or packs one plane element to the wrong place is wrong by 2^-17 .. 2^-9 of that output, against a correct kernel's
few 2^-24. Plain numpy, no GPU:

  weight_probes      dense weights, input zero except on a pixel lattice no output window sees twice, one non-zero channel per lattice pixel
  activation_probes  dense input, one non-zero weight per output channel
  Probe.check        element-wise |got - exact| <= 4 * 2^-24 * (|x * w| + |bias|) in float64, exact zeros where no term lands
  coverage           which weight / input elements were the non-zero factor of a checked non-zero output; the generators add passes
                     until it is full, the tests assert that it is
  emulate            the six-product scheme as the kernels do it (round-to-nearest-even split, the order of mma_step3, f32 accumulate
                     rounding to nearest or truncating), with optional injected defects - the proof that the bound separates right from wrong

The bound (4 u, u = 2^-24) follows from the arithmetic, not from a kernel: the five small products are added first, their roundings are
below 2^-32 of the result; the last add (hh) rounds once, at most one f32 ulp = 2 u when the adder truncates; the dropped ml / lm / ll
products are below 2^-26. A kernel on the f32 MFMA or FMA rounds once: <= 1 u.
"""
import numpy as np

U = 2.0 ** -24
BOUND_U = 4.0

# (N, H, W, C, K, k, pad, stride, dil): every convolution geometry the GPU probe test runs (the CPU test proves the probes on the same list)
CONV_GEOMETRIES = {
    "res2_3x3": (2, 28, 28, 64, 64, 3, 1, 1, 1),
    "res4_3x3_n8": (8, 14, 14, 256, 256, 3, 1, 1, 1),       # split-K eligible at N = 8
    "pw_c64_k256": (2, 14, 14, 64, 256, 1, 0, 1, 1),
    "pw_c128_k512": (1, 14, 14, 128, 512, 1, 0, 1, 1),
    "pw_c256_k64": (2, 14, 14, 256, 64, 1, 0, 1, 1),
    "c48_k34": (1, 7, 7, 48, 34, 3, 1, 1, 1),               # a 32-deep slab straddles taps, K % 4 != 0
    "c16_dil2": (1, 10, 10, 16, 16, 3, 2, 1, 2),
    "stride2_13x11": (2, 13, 11, 32, 64, 3, 1, 2, 1),
    "k5_nchw": (1, 5, 5, 64, 32, 5, 2, 1, 1),
    "ragged_3x3": (2, 19, 23, 64, 128, 3, 1, 1, 1),         # partial pixel tiles, the halo kernels' edge rows
    "ragged_1x1": (1, 19, 23, 64, 64, 1, 0, 1, 1),
}
POOL2_GEOMETRIES = {"res2_3x3": (2, 28, 28, 64, 64, 3, 1, 1, 1), "res4_3x3": (2, 14, 14, 256, 256, 3, 1, 1, 1)}
# (N, H, W, C, K1, K2, k, pad, stride): test_conv_f32_sibling_pair_equals_two_ops's shapes
PAIR_GEOMETRIES = [(2, 14, 14, 64, 256, 64, 1, 0, 1), (1, 9, 7, 128, 128, 48, 1, 0, 2), (1, 6, 6, 32, 128, 16, 3, 1, 1)]
STEM_IMAGES = [(1, 224, 224), (1, 61, 47), (2, 33, 40)]
GEMM_SHAPES = [(333, 200, 264), (16, 515, 4104)]            # (m, n, k)
FC_SHAPES = [(8, 2048, 1000), (3, 512, 40)]                 # (m, k, n)
SCALE_SHIFTS = [(60, 0), (-60, 0), (0, 60), (0, -60)]       # binades added to every exponent of (input, weights): products stay inside 2^+-86


def stem_geometry(n, h, w):
    return (n, h, w, 3, 64, 7, 3, 2, 1)


def gemm_geometry(m, n, k):
    """C[m][n] = A[m][k] . B[k][n] as a 1x1 convolution on m one-pixel images: A is the input, B's columns are the output channels."""
    return (m, 1, 1, k, n, 1, 0, 1, 1)


def out_hw(geo):
    N, H, W, C, K, k, pad, stride, dil = geo
    span = dil * (k - 1) + 1
    return (H + 2 * pad - span) // stride + 1, (W + 2 * pad - span) // stride + 1


def rand_f32(rng, shape, shift=0, binades=13, sign=None):
    """f32 values with a full random 24-bit mantissa, exponents uniform over `binades` binades around 2^shift, random sign (or `sign`)."""
    mant = (1 << 23) + rng.integers(0, 1 << 23, shape)
    e = rng.integers(-(binades // 2), binades - binades // 2, shape) + shift
    v = np.ldexp(mant.astype(np.float64), e - 23)
    v = v * (rng.choice([-1.0, 1.0], shape) if sign is None else sign)
    r = v.astype(np.float32)
    assert np.array_equal(r.astype(np.float64), v)
    return r


def _pool_dim(n, win, stride, ceil_mode):
    if not ceil_mode:
        return (n - win) // stride + 1
    o = -(-(n - win) // stride) + 1
    return o - 1 if (o - 1) * stride >= n else o


def _pool_max(a, pool):
    """max pooling of a [N, K, oh, ow] array, unpadded; windows clipped at the edge (ceil shapes)"""
    win, stride, ceil_mode = pool
    oh, ow = a.shape[2:]
    ph, pw = _pool_dim(oh, win, stride, ceil_mode), _pool_dim(ow, win, stride, ceil_mode)
    out = np.full(a.shape[:2] + (ph, pw), -np.inf, a.dtype)
    for di in range(win):
        rows = np.arange(ph) * stride + di
        rows = rows[rows < oh]
        for dj in range(win):
            cols = np.arange(pw) * stride + dj
            cols = cols[cols < ow]
            v = a[:, :, rows][:, :, :, cols]
            np.maximum(out[:, :, :len(rows), :len(cols)], v, out=out[:, :, :len(rows), :len(cols)])
    return out


class Probe:
    """One pass: the tensors of one launch, the single term of every non-zero output, and the exact answer.

    x [N, C, H, W], w [K, C, k, k], bias [K] or None (f32). Term t: conv output element out_idx[t] (flat in [N, K, oh, ow]) is
    x.flat[x_idx[t]] * w.flat[w_idx[t]]; every other conv output has no term. relu / pool = (window, stride, ceil_mode): what the probed op
    applies behind the convolution. w_exact: the f32 weights the kernel really multiplies when they differ from w (a GEMM's alpha)."""

    def __init__(self, geo, x, w, bias, out_idx, x_idx, w_idx, relu=False, pool=None, w_exact=None):
        self.geo, self.x, self.w, self.bias, self.relu, self.pool = geo, x, w, bias, relu, pool
        self.out_idx, self.x_idx, self.w_idx = out_idx, x_idx, w_idx
        self.w_exact = w if w_exact is None else w_exact
        N, H, W, C, K, k, pad, stride, dil = geo
        oh, ow = out_hw(geo)
        self.conv_shape = (N, K, oh, ow)
        assert len(np.unique(out_idx)) == len(out_idx), "two terms in one output"
        assert not (pool and not relu) and not (relu and bias is not None)
        term = self.x.astype(np.float64).ravel()[x_idx] * self.w_exact.astype(np.float64).ravel()[w_idx]      # exact: 48 bits
        self.term = term
        e = np.zeros(self.conv_shape, np.float64)
        e.ravel()[out_idx] = term
        mag = np.abs(e)
        if bias is not None:
            b = bias.astype(np.float64)[None, :, None, None]
            e = e + b
            mag = mag + np.abs(b)
        if relu:
            e = np.maximum(e, 0.0)
            mag = e
        if pool:
            e = _pool_max(e, pool)
            mag = e
        self.exact = e
        self.bound = BOUND_U * U * mag

    def coverage(self):
        """(weight mask [K, C, k, k], input mask [N, C, H, W]): elements that were the factor of a checked, non-zero output"""
        ok = self.term != 0.0
        if self.relu:
            ok &= self.term > 0.0
        if self.pool:
            win, stride, _ = self.pool
            ph, pw = self.exact.shape[2:]
            n, k, oy, ox = np.unravel_index(self.out_idx, self.conv_shape)
            surv = np.zeros(len(self.term), bool)
            for di in range(win):
                for dj in range(win):
                    py, px = oy - di, ox - dj
                    v = (py >= 0) & (px >= 0) & (py % stride == 0) & (px % stride == 0)
                    py, px = py // stride, px // stride
                    v &= (py < ph) & (px < pw)
                    s = np.zeros(len(self.term), bool)
                    s[v] = self.exact[n[v], k[v], py[v], px[v]] == self.term[v]
                    surv |= s
            ok &= surv
        wm = np.zeros(self.w.size, bool)
        xm = np.zeros(self.x.size, bool)
        wm[self.w_idx[ok]] = True
        xm[self.x_idx[ok]] = True
        return wm.reshape(self.w.shape), xm.reshape(self.x.shape)

    def apply(self, product):
        """The op's f32 output [N, K, OH, OW] when every term is computed by product(x_idx, w_idx) -> f32 and every other product is zero"""
        out = np.zeros(self.conv_shape, np.float32)
        out.ravel()[self.out_idx] = product(self.x_idx, self.w_idx)
        if self.bias is not None:
            out = out + self.bias[None, :, None, None]       # f32 add in the epilogue
        if self.relu:
            out = np.maximum(out, np.float32(0))
        if self.pool:
            out = _pool_max(out, self.pool)
        return out

    def failures(self, got):
        got = np.asarray(got)
        assert got.shape == self.exact.shape, (got.shape, self.exact.shape)
        err = np.abs(got.astype(np.float64) - self.exact)
        return np.argwhere(~(err <= self.bound))      # (NaN fails; where the bound is 0 the output must be 0, either sign)

    def check(self, got, what=""):
        bad = self.failures(got)
        if len(bad) == 0:
            return
        err = np.abs(np.asarray(got, np.float64) - self.exact)
        N, H, W, C, K, k, pad, stride, dil = self.geo
        term_of = {}
        if not self.pool:
            term_of = dict(zip(self.out_idx.tolist(), range(len(self.out_idx))))
        lines = []
        for idx in bad[:12]:
            idx = tuple(int(i) for i in idx)
            g, e = float(np.asarray(got)[idx]), float(self.exact[idx])
            t = term_of.get(int(np.ravel_multi_index(idx, self.exact.shape)))
            src = ""
            if t is not None:
                kk, c, i, j = np.unravel_index(self.w_idx[t], self.w.shape)
                n, c2, py, px = np.unravel_index(self.x_idx[t], self.x.shape)
                src = " term w[k=%d, c=%d, tap=(%d, %d)] * x[n=%d, c=%d, y=%d, x=%d]" % (kk, c, i, j, n, c2, py, px)
            rel = err[idx] / abs(e) / U if e != 0.0 else float("inf")
            lines.append("  out[n, k, y, x] = %s: got %.9g exact %.9g error %.1f u (log2 rel %.1f)%s" %
                         (idx, g, e, rel, np.log2(max(rel * U, 1e-300)), src))
        raise AssertionError("%s: %d of %d outputs outside %g u%s\n%s" % (what, len(bad), self.exact.size, BOUND_U,
                                                                          " (geometry %s)" % (self.geo,), "\n".join(lines)))


class ProbeSet:
    """passes + the coverage they reach: wcov [K, C, k, k], xcov [N, C, H, W], poscov [C, k, k] (positions a sparse weight set covered)"""

    def __init__(self, geo, family):
        self.geo, self.family, self.passes = geo, family, []
        N, H, W, C, K, k, pad, stride, dil = geo
        self.wcov = np.zeros((K, C, k, k), bool)
        self.xcov = np.zeros((N, C, H, W), bool)
        # input elements the convolution reads at all (a 1x1 / stride-2 conv never reads the odd pixels): what "every input element" means
        oh, ow = out_hw(geo)
        ry, rx = np.zeros(H, bool), np.zeros(W, bool)
        for i in range(k):
            iy, ix = np.arange(oh) * stride - pad + i * dil, np.arange(ow) * stride - pad + i * dil
            ry[iy[(iy >= 0) & (iy < H)]] = True
            rx[ix[(ix >= 0) & (ix < W)]] = True
        self.xread = np.broadcast_to((ry[:, None] & rx[None, :])[None, None], (N, C, H, W))

    def add(self, p):
        self.passes.append(p)
        wm, xm = p.coverage()
        self.wcov |= wm
        self.xcov |= xm

    @property
    def poscov(self):
        return self.wcov.any(axis=0)


_PARITIES = [(0, 0), (0, 1), (1, 0), (1, 1)]


def weight_probes(geo, rng, shift=(0, 0), bias=False, pool2=False, w_alpha=None, max_passes=4000):
    """Dense weights, sparse input; passes are added (lattice origin shifted, channel walk continued) until every weight element is covered.

    pool2: the op is conv + relu + 2x2 / 2 max pooling. A pooling window holds up to four taps of one lattice pixel, so only one may
    survive the relu: four weight sets, set (a, b) has the sign that makes the product positive on the taps of parity (a, b) and the
    opposite sign elsewhere (signs still random per channel: sign(x) = s[c], sign(w[k, c, tap]) = +-s[c]); lattice spacing 4, so that
    two lattice pixels never meet in one window."""
    N, H, W, C, K, k, pad, stride, dil = geo
    oh, ow = out_hw(geo)
    span = dil * (k - 1) + 1
    S = span + (1 if span % 2 else 2) if pool2 else span      # pool2: even and wider than a window's reach
    ps = ProbeSet(geo, "weight")
    origins = [(a, b) for a in range(S) for b in range(S)]
    origins = [origins[0]] + [origins[i] for i in rng.permutation(np.arange(1, len(origins)))]
    q = 0
    classes = [cl for cl in _PARITIES if cl[0] < k and cl[1] < k] if pool2 else [None]
    for cl in classes:
        sig = rng.choice([-1.0, 1.0], C)
        if cl is None:
            w = rand_f32(rng, (K, C, k, k), shift[1])
            want = np.ones((K, C, k, k), bool)
        else:
            tapsel = ((np.arange(k)[:, None] % 2 == cl[0]) & (np.arange(k)[None, :] % 2 == cl[1]))
            w = rand_f32(rng, (K, C, k, k), shift[1], sign=sig[None, :, None, None] * np.where(tapsel, 1.0, -1.0)[None, None])
            want = np.broadcast_to(tapsel[None, None], (K, C, k, k))
        b = rand_f32(rng, (K,), shift[0] + shift[1]) if bias else None
        w_exact = None if w_alpha is None else (np.float32(w_alpha) * w).astype(np.float32)
        for t in range(max_passes):
            if (ps.wcov | ~want).all():
                break
            a0, b0 = origins[t % len(origins)]
            ys, xs = np.arange(a0, H, S), np.arange(b0, W, S)
            if len(ys) == 0 or len(xs) == 0:
                continue
            n_i, py, px = [v.ravel() for v in np.meshgrid(np.arange(N), ys, xs, indexing="ij")]
            T = len(n_i)
            ch = (q + np.arange(T)) % C
            q += T + (1 if T % C == 0 else 0)
            x = np.zeros((N, C, H, W), np.float32)
            x[n_i, ch, py, px] = rand_f32(rng, (T,), shift[0], sign=None if cl is None else sig[ch])
            oi, xi, wi = [], [], []
            karr = np.arange(K)[None, :]
            for i in range(k):
                ty = py + pad - i * dil
                for j in range(k):
                    tx = px + pad - j * dil
                    v = (ty >= 0) & (tx >= 0) & (ty % stride == 0) & (tx % stride == 0) & (ty // stride < oh) & (tx // stride < ow)
                    if not v.any():
                        continue
                    oy, ox = (ty[v] // stride)[:, None], (tx[v] // stride)[:, None]
                    oi.append((((n_i[v][:, None] * K + karr) * oh + oy) * ow + ox).ravel())
                    xi.append(np.broadcast_to((((n_i[v] * C + ch[v]) * H + py[v]) * W + px[v])[:, None], (int(v.sum()), K)).ravel())
                    wi.append((((karr * C + ch[v][:, None]) * k + i) * k + j).ravel())
            ps.add(Probe(geo, x, w, b, np.concatenate(oi), np.concatenate(xi), np.concatenate(wi), relu=pool2,
                         pool=(2, 2, False) if pool2 else None, w_exact=w_exact))
        else:
            raise AssertionError("weight probes: coverage not full after %d passes (%s)" % (max_passes, geo))
    return ps


def activation_probes(geo, rng, shift=(0, 0), bias=False, pool2=False, stem=False, max_sets=4000):
    """Dense input, one non-zero weight per output channel at a position that walks over all C * k * k positions across the channels and
    the weight sets; sets are added until every position was used and every input element is covered.

    pool2 (conv + relu + 2x2 / 2 max pooling): a window holds one input pixel of each parity under any tap, so every weight set runs on
    four inputs, input (a, b) positive-product on the pixels of parity (a, b) only. stem (7x7 / 2 conv + relu + 3x3 / 2 max pooling,
    ceil shapes): positive inputs and weights, the coverage asked for is that of the 147 positions (poscov)."""
    N, H, W, C, K, k, pad, stride, dil = geo
    oh, ow = out_hw(geo)
    npos = C * k * k
    ps = ProbeSet(geo, "activation")
    pool = (2, 2, False) if pool2 else ((3, 2, True) if stem else None)
    oy, ox = np.arange(oh), np.arange(ow)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    s = 0
    while True:
        done_pos = s * K >= npos
        if done_pos and (ps.poscov.all() if stem else (ps.xcov | ~ps.xread).all()):
            break
        if s >= max_sets:
            raise AssertionError("activation probes: coverage not full after %d weight sets (%s)" % (max_sets, geo))
        pos = (s * K + np.arange(K)) % npos
        tap, c_k = pos // C, pos % C                       # channel fastest: one weight set spans many channels
        i_k, j_k = tap // k, tap % k
        sig = rng.choice([-1.0, 1.0], C)
        w = np.zeros((K, C, k, k), np.float32)
        w[np.arange(K), c_k, i_k, j_k] = rand_f32(rng, (K,), shift[1], sign=1.0 if stem else (sig[c_k] if pool2 else None))
        b = rand_f32(rng, (K,), shift[0] + shift[1]) if bias else None
        iy = oy[None, :] * stride - pad + i_k[:, None] * dil          # [K, oh]
        ix = ox[None, :] * stride - pad + j_k[:, None] * dil          # [K, ow]
        valid = ((iy >= 0) & (iy < H))[:, :, None] & ((ix >= 0) & (ix < W))[:, None, :]      # [K, oh, ow]
        kk, vy, vx = np.nonzero(valid)
        nn = np.arange(N)[:, None]
        out_idx = (((nn * K + kk[None]) * oh + vy[None]) * ow + vx[None]).ravel()
        x_idx = (((nn * C + c_k[kk][None]) * H + iy[kk, vy][None]) * W + ix[kk, vx][None]).ravel()
        w_idx = np.broadcast_to(np.ravel_multi_index((kk, c_k[kk], i_k[kk], j_k[kk]), w.shape)[None], (N, len(kk))).ravel()
        for cl in (_PARITIES if pool2 else [None]):
            if cl is None:
                x = rand_f32(rng, (N, C, H, W), shift[0], sign=1.0 if stem else None)
            else:
                par = np.where((yy % 2 == cl[0]) & (xx % 2 == cl[1]), 1.0, -1.0)
                x = rand_f32(rng, (N, C, H, W), shift[0], sign=sig[None, :, None, None] * par[None, None])
            ps.add(Probe(geo, x, w, b, out_idx, x_idx, w_idx, relu=pool is not None, pool=pool))
        s += 1
    return ps


# ---- the six-product scheme on the CPU -------------------------------------------------------------------------------------------------
def split3(v):
    """f32 -> (h, m, l) bf16 planes as f32 arrays: round to nearest even, exact residuals (split3_pair, conv_igemm_impl.h; the host and
    device weight packers do the same on integers)"""
    def rne(a):
        u = np.ascontiguousarray(a, np.float32).view(np.uint32)
        return ((u + np.uint32(0x7fff) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xffff0000)).view(np.float32)
    v = np.ascontiguousarray(v, np.float32)
    h = rne(v)
    r1 = v - h
    m = rne(r1)
    r2 = r1 - m
    return np.stack([h, m, rne(r2)])


MMA_ORDER = ((2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0))      # mma_step3: (weight plane, input plane), small terms first
DEFECTS = ("w_no_l", "no_mm", "no_lh", "w_swap_l", "w_m_neighbour", "x_swap_l", "x_m_neighbour")
WEIGHT_SIDE = ("w_no_l", "no_mm", "no_lh", "w_swap_l", "w_m_neighbour")      # what the weight probes must catch
INPUT_SIDE = ("no_mm", "no_lh", "x_swap_l", "x_m_neighbour")                  # what the activation probes must catch


def _round_f32(s, trunc):
    r = s.astype(np.float32)
    if trunc:
        over = np.abs(r.astype(np.float64)) > np.abs(s)
        r = np.where(over, np.nextafter(r, np.float32(0)), r)
    return r


_planes_of = [None, None]      # the passes of a weight-probe set share one dense weight tensor: split it once


def _weight_planes(w):
    if _planes_of[0] is not w:
        _planes_of[:] = [w, split3(w)]
    return _planes_of[1]


def emulate(p, trunc=False, defect=None, k0=0):
    """probe p through the six-product scheme: f32 output [N, K, OH, OW]. trunc: every f32 accumulate truncates (the pessimistic model of
    the MFMA adder) instead of rounding to nearest. defect: one of DEFECTS (w_swap_l: in output channel k0)."""
    wp, xp = _weight_planes(p.w_exact), split3(p.x)
    if defect in ("w_no_l", "w_swap_l", "w_m_neighbour"):
        wp = wp.copy()
    skip = {"no_mm": (1, 1), "no_lh": (2, 0)}.get(defect)
    if defect == "w_no_l":
        wp[2] = 0
    elif defect == "w_swap_l":          # two neighbouring channels of one (k, tap): a fragment packer off by one element
        a = wp[2][k0, 0, 0, 0].copy()
        wp[2][k0, 0, 0, 0] = wp[2][k0, 1, 0, 0]
        wp[2][k0, 1, 0, 0] = a
    elif defect == "w_m_neighbour":
        wp[1][:, 0] = wp[1][:, 1]
    elif defect == "x_swap_l":
        a = xp[2][0, 0].copy()
        xp[2][0, 0] = xp[2][0, 1]
        xp[2][0, 1] = a
    elif defect == "x_m_neighbour":
        xp[1][:, 0] = xp[1][:, 1]
    wp, xp = wp.reshape(3, -1), xp.reshape(3, -1)

    def product(x_idx, w_idx):
        acc = np.zeros(len(x_idx), np.float32)
        for pw, px in MMA_ORDER:
            if (pw, px) == skip:
                continue
            acc = _round_f32(acc.astype(np.float64) + wp[pw][w_idx].astype(np.float64) * xp[px][x_idx].astype(np.float64), trunc)
        return acc
    return p.apply(product)


def dense_inputs(geo, rng):
    """both signs, exponents over 12 binades, full mantissas: the inputs of the dense accumulation statistic"""
    N, H, W, C, K, k, pad, stride, dil = geo
    return rand_f32(rng, (N, C, H, W), binades=12), rand_f32(rng, (K, C, k, k), binades=12)


def dense_exact(geo, x, w):
    """(exact float64 convolution, sum |x| |w|) of a stride-1 / dilation-1 geometry, [N, K, oh, ow]"""
    N, H, W, C, K, k, pad, stride, dil = geo
    assert stride == 1 and dil == 1
    oh, ow = out_hw(geo)
    xp = np.zeros((N, C, H + 2 * pad, W + 2 * pad), np.float64)
    xp[:, :, pad:pad + H, pad:pad + W] = x
    w64 = w.astype(np.float64)
    e = np.zeros((N, K, oh, ow), np.float64)
    a = np.zeros((N, K, oh, ow), np.float64)
    for i in range(k):
        for j in range(k):
            xs = xp[:, :, i:i + oh, j:j + ow]
            e += np.einsum("nchw,kc->nkhw", xs, w64[:, :, i, j])
            a += np.einsum("nchw,kc->nkhw", np.abs(xs), np.abs(w64[:, :, i, j]))
    return e, a


DENSE_GEOMETRIES = {64: (2, 12, 12, 64, 64, 1, 0, 1, 1), 576: (2, 12, 12, 64, 64, 3, 1, 1, 1), 1152: (2, 12, 12, 128, 64, 3, 1, 1, 1)}
# the smallest ratio (statistic of an emulated defect / the oracle's) that tests/test_fp32_probe_cpu.py finds per reduction length, rounded down
DENSE_DEFECT_FLOOR = {64: 14.5, 576: 5.3, 1152: 3.7}
DENSE_DEFECTS = ("w_no_l", "no_mm", "no_lh")      # the defects that touch every output (a packing slip of two elements does not move an RMS)


def dense_stat(got, exact, absum):
    """RMS over the outputs of |got - exact| / sum |x| |w|, in units of u = 2^-24"""
    r = (np.asarray(got, np.float64) - exact) / absum
    return float(np.sqrt(np.mean(r * r)) / U)


def emulate_dense(geo, x, w, trunc=False, defect=None):
    """The six-product scheme on a dense stride-1 convolution with C % 32 == 0: reduction index (tap, channel) in 32-deep slabs, per slab
    the six plane products in the order of mma_step3, each one exact 32-term sum rounded into the f32 accumulator (one rounding per MFMA)."""
    N, H, W, C, K, k, pad, stride, dil = geo
    assert stride == 1 and dil == 1 and C % 32 == 0
    oh, ow = out_hw(geo)
    wp, xs = split3(w).astype(np.float64), split3(x).astype(np.float64)
    if defect == "w_no_l":
        wp[2] = 0
    skip = {"no_mm": (1, 1), "no_lh": (2, 0)}.get(defect)
    xp = np.zeros((3, N, C, H + 2 * pad, W + 2 * pad), np.float64)
    xp[:, :, :, pad:pad + H, pad:pad + W] = xs
    acc = np.zeros((N, K, oh, ow), np.float32)
    for i in range(k):
        for j in range(k):
            for c0 in range(0, C, 32):
                for pw, px in MMA_ORDER:
                    if (pw, px) == skip:
                        continue
                    part = np.einsum("nchw,kc->nkhw", xp[px][:, c0:c0 + 32, i:i + oh, j:j + ow], wp[pw][:, c0:c0 + 32, i, j])
                    acc = _round_f32(acc.astype(np.float64) + part, trunc)
    return acc


# ---- the cases both test files run: the CPU test proves the probes (emulation, oracle, injected defects), the GPU test runs the kernels ----
def _seed(name):
    return int.from_bytes(name.encode(), "little") % (2 ** 31)


def case_list():
    """name -> (geometry, keyword arguments of the two generators, families)"""
    cases = {}
    for name, geo in CONV_GEOMETRIES.items():
        cases["conv/" + name] = (geo, {}, ("weight", "activation"))
    for name in ("res2_3x3", "pw_c64_k256", "pw_c128_k512"):       # one bias case per form: implicit GEMM / halo, pointwise kernels
        cases["bias/" + name] = (CONV_GEOMETRIES[name], {"bias": True}, ("weight", "activation"))
    for name in ("res2_3x3", "pw_c64_k256"):
        for sx, sw in SCALE_SHIFTS:
            cases["scale/%s/%+d%+d" % (name, sx, sw)] = (CONV_GEOMETRIES[name], {"shift": (sx, sw)}, ("weight", "activation"))
    for name, geo in POOL2_GEOMETRIES.items():
        cases["pool2/" + name] = (geo, {"pool2": True}, ("weight", "activation"))
    for (N, H, W, C, K1, K2, k, pad, stride) in PAIR_GEOMETRIES:
        # a sibling pair is the convolution with the two ops' output channels concatenated
        cases["pair/%dx%dx%d_c%d_k%d+%d" % (N, H, W, C, K1, K2)] = ((N, H, W, C, K1 + K2, k, pad, stride, 1), {}, ("weight", "activation"))
    for img in STEM_IMAGES:
        cases["stem/%dx%dx%d" % img] = (stem_geometry(*img), {"stem": True}, ("activation",))
    for (m, n, k) in GEMM_SHAPES:
        cases["gemm/%dx%dx%d" % (m, n, k)] = (gemm_geometry(m, n, k), {}, ("weight", "activation"))
    m, n, k = GEMM_SHAPES[0]
    cases["gemm_alpha/%dx%dx%d" % (m, n, k)] = (gemm_geometry(m, n, k), {"w_alpha": 0.7}, ("weight",))
    for (m, k, n) in FC_SHAPES:
        cases["fc/%dx%dx%d" % (m, k, n)] = (gemm_geometry(m, n, k), {"bias": True}, ("activation",))
    return cases


def build_case(name):
    """the ProbeSets of a case, by family; the same seed gives the CPU test and the GPU test the same probes"""
    geo, kw, families = case_list()[name]
    rng = np.random.default_rng(_seed(name))
    out = {}
    if "weight" in families:
        out["weight"] = weight_probes(geo, rng, **{k: v for k, v in kw.items() if k != "stem"})
    if "activation" in families:
        out["activation"] = activation_probes(geo, rng, **{k: v for k, v in kw.items() if k != "w_alpha"})
    return out


def assert_full_coverage(ps, stem=False):
    if ps.family == "weight":
        assert ps.wcov.all(), ("weight probes: %d weight elements never the factor of a checked output" % (~ps.wcov).sum(), ps.geo)
    elif stem:
        assert ps.poscov.all(), ("stem probes: (c, tap) positions not covered", np.argwhere(~ps.poscov)[:8], ps.geo)
    else:
        assert np.array_equal(ps.xcov, ps.xread), ("activation probes: %d input elements that the convolution reads were never the factor "
                                                   "of a checked output" % (ps.xread & ~ps.xcov).sum(), ps.geo)
        assert ps.poscov.all(), ("activation probes: (c, tap) positions never used", ps.geo)
