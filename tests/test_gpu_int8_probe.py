"""The INT8 requantisation probes (tests/int8_probe.py) through every accepted kernel form: exact ties of both parities and signs, both
rails, +-1e6, accumulators beyond 2^24 and the searched accumulators at which a contracted or reassociated epilogue rounds to another byte -
against the oracle, byte for byte. The random-data parity tests essentially never put a pre-rounding value within an ulp of m + 0.5;
tests/test_int8_probe_cpu.py proves on the CPU that these probes do, and that each named defect changes a byte of them."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from anakin_amd import lib as L  # noqa: E402
from anakin_amd import saber as S  # noqa: E402
from oracle import oracle as O  # noqa: E402
from tests import int8_probe as P  # noqa: E402

from tests.test_gpu_parity import _I8_CODES as I8_CODES  # noqa: E402  (every selection code the library might accept for an INT8 conv)

SENTINEL = 77
GROUPS = P.group_list()


@pytest.fixture(scope="module", autouse=True)
def _device():
    L.require_device()  # fail loudly: no fallback path exists


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _forms(op):
    """[(code, algo name)]: the selection the op starts with, then every code set_tile accepts, one per kernel name"""
    forms = [(L.load().saber_hip_conv2d_get_tile(op.h), op.algo())]
    seen = {op.algo()}
    for code in I8_CODES:
        try:
            op.set_tile(code)
        except L.SaberHipError:
            continue
        if op.algo() not in seen:
            seen.add(op.algo())
            forms.append((code, op.algo()))
    op.set_tile(forms[0][0])
    assert op.algo() == forms[0][1], (op.algo(), forms[0])
    return forms


def check(p, got, want, what):
    """np.array_equal with the form, the class and the first bad index in the message"""
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if np.array_equal(got, want):
        return
    bad = np.argwhere(got != want)
    i = tuple(int(v) for v in bad[0])
    raise AssertionError("%s: %s: %d of %d bytes differ, first at [n, y, x, k] = %s: got %d, oracle %d (%s)" %
                         (p.name if p is not None else "-", what, len(bad), want.size, i, int(got[i]), int(want[i]),
                          P.describe(p, i) if p is not None else ""))


def make_conv(p, **kw):
    """the library op of probe p (s8 weights with their explicit w_scale, as run_conv_i8 passes them)"""
    N, H, W, C, K, k, pad, stride = p.geo
    cp = S.ConvParam(p.wq, p.bias, 1, (pad, pad), (stride, stride), (1, 1), p.relu, p.w_scale)
    if p.mode == "elt":
        res, res_relu, coeff, s1 = p.elt
        cp.res_mode, cp.res_relu, cp.sum_scale, cp.coeff, cp.scale_res = L.RES_ELTWISE, res_relu, 1.0, coeff, s1
    elif p.mode == "sum":
        cp.res_mode, cp.res_relu, cp.sum_scale, cp.res_dtype = L.RES_SUM_INPLACE, False, p.sum[1], p.meta["rdt"]
    return S.SaberConv2D(int8=True).init((N, C, H, W), cp, p.idt, p.odt, p.in_scale, p.out_scale, **kw)


# the kernel forms that refuse a fused mode (set_tile answers an error on an op in that mode), by group: the image-resident kernel has
# no in-place sum. Asserted, so that a form that starts or stops refusing is noticed.
REFUSES = {"sum/imgres1x1": {"imgres1x1_i8_16ch"}, "sum/imgres3x3": {"imgres3x3_i8_16ch"}}


def run_forms(p, forms_seen):
    """probe p through the static selection and every accepted code; returns the number of launches. Nothing is caught here: an op
    that cannot be created in the probe's mode, or a launch that answers an error, fails the test."""
    want = P.oracle_bytes(p)
    conv = make_conv(p)
    xd = dev(p.x)
    rd = dev(p.elt[0]) if p.mode == "elt" else None
    prev = dev(p.sum[0].view(P.NP_DT[p.odt])) if p.mode == "sum" else None
    forms = _forms(conv)
    for code, algo in forms:
        conv.set_tile(code)
        assert conv.algo() == algo, (conv.algo(), algo)
        y = conv.new_output()
        if prev is not None:
            y.copy_(prev)
        else:
            y.fill_(SENTINEL)
        conv.dispatch(xd, y, rd)
        check(p, host(y), want, "%s (%s)" % (algo, hex(code)))
        forms_seen.add(algo)
    return len(forms)


@pytest.mark.parametrize("group", sorted(g for g in GROUPS if not g.startswith(("stempool/", "dw/"))))
def test_conv_i8_probes_every_accepted_form(group):
    """Plain convolutions (all four 8-bit dtype combinations, relu on and off), the fused eltwise (four coefficient sets), the in-place sum
    (sum_scale 1 and not 1, the bytes in y of either dtype) and the accumulators beyond 2^24, on 1x1 (K 64 / 72 / 34), 3x3 (halo and
    image-resident) and the 7x7 / 2 stem: the static selection and every accepted selection code, one run per kernel name."""
    seen, runs = set(), 0
    for name in GROUPS[group]:
        p = P.build(name)
        P.assert_classes(p)
        runs += run_forms(p, seen)
    assert seen and runs, group
    if group.startswith("elt/"):                # three (relu, res_relu) settings x every coefficient set, the three with c0 != c1 among them
        n_new = sum(name.rsplit("/", 1)[1] in P.COEFF_MODES for name in GROUPS[group])
        assert len(GROUPS[group]) == 3 * len(P.ELT_MODES) and n_new == 9, (group, len(GROUPS[group]), n_new)
        print("%s: %d elt probes, %d of them with c0 != c1" % (group, len(GROUPS[group]), n_new))
    if group.startswith(("elt/", "sum/")):      # the forms of the plain conv on this geometry that this mode does not have
        plain = {a for _, a in _forms(make_conv(P.build("conv/%s/u8u8/relu1" % group.split("/")[1])))}
        key = "/".join(group.split("/")[:2])
        assert plain - seen == REFUSES.get(key, set()) and seen <= plain, (group, sorted(plain - seen), sorted(seen - plain))
        print("%s: forms that refuse this mode: %s" % (group, sorted(plain - seen) or "none"))
    print("%s: %d probes, %d launches, %d kernel forms: %s" % (group, len(GROUPS[group]), runs, len(seen), " ".join(sorted(seen))))


def test_conv_i8_probe_geometries_reach_every_form_family():
    """The geometries above reach every family of INT8 convolution kernels."""
    seen = set()
    for gn in P.GEOMETRIES:
        seen |= {a for _, a in _forms(make_conv(P.build("conv/%s/u8u8/relu1" % gn)))}
    seen |= {a for _, a in _forms(make_conv(P.build("elt/pw_k64/u8/relu0_res1/half")))}
    want = {"implicit GEMM": [a for a in seen if a.startswith("igemm_i8")], "halo 3x3": [a for a in seen if a.startswith("halo3x3_i8")],
            "image-resident 3x3": [a for a in seen if a.startswith("img3x3_i8")], "stem": [a for a in seen if a.startswith("stem7x7s2_i8")],
            "image-resident 1x1": [a for a in seen if a.startswith("imgres1x1_i8")],
            "image-resident 3x3 (whole image)": [a for a in seen if a.startswith("imgres3x3_i8")]}
    print({k: len(v) for k, v in want.items()}, sorted(seen))
    assert all(want.values()), {k: len(v) for k, v in want.items()}


# ---- sibling pair ------------------------------------------------------------------------------------------------------------------------
PAIR_GEO = (1, 6, 6, 32, 128, 32, 3, 1, 1)       # tests/test_gpu_parity.py's smallest PAIR_CASES entry with K2 = 32 instead of 16: 15 channel kinds, each twice


@pytest.mark.parametrize("idt", [P.S8, P.U8])
@pytest.mark.parametrize("first", [P.S8, P.U8])
def test_conv_i8_sibling_pair_probes(idt, first):
    """Two convs over one input in one launch (epilogue_i8_pair: clamp and offset chosen at run time): s8 and u8 on either side, relu on
    the u8 side, both outputs against the oracle, every accepted form."""
    N, H, W, C, K1, K2, k, pad, stride = PAIR_GEO
    second = P.U8 if first == P.S8 else P.S8
    pa = P.build("conv/pair/%s%s/relu%d" % (P.DT_NAME[idt], P.DT_NAME[first], first == P.U8), (N, H, W, C, K1, k, pad, stride))
    pb = P.build("conv/pair/%s%s/relu%d" % (P.DT_NAME[idt], P.DT_NAME[second], second == P.U8), (N, H, W, C, K2, k, pad, stride))
    assert np.array_equal(pa.x, pb.x), "the two probes must read one input"
    P.assert_classes(pa)
    P.assert_classes(pb)
    a, b = make_conv(pa), make_conv(pb)
    pair = S.SaberConvPair(a, b)
    forms = _forms(pair)
    assert all(n.startswith("pair_igemm_i8") for _, n in forms), forms
    xd = dev(pa.x)
    for code, algo in forms:
        pair.set_tile(code)
        ya, yb = a.new_output(), b.new_output()
        ya.fill_(SENTINEL)
        yb.fill_(SENTINEL)
        pair.dispatch(xd, ya, yb)
        check(pa, host(ya), P.oracle_bytes(pa), "first output, %s (%s)" % (algo, hex(code)))
        check(pb, host(yb), P.oracle_bytes(pb), "second output, %s (%s)" % (algo, hex(code)))
    print("pair %s -> %s + %s: %d forms: %s" % (P.DT_NAME[idt], P.DT_NAME[first], P.DT_NAME[second], len(forms), " ".join(n for _, n in forms)))


# ---- 1x1 chain ---------------------------------------------------------------------------------------------------------------------------
CHAIN_CASES = [(64, 9, None), (64, 9, 2), (64, 9, 4), (256, 5, 9), (256, 5, 11)]       # C, H = W, pixel-tile code


def _random_conv(rng, shape_in, K, idt, odt, relu, in_scale, out_scale):
    """an ordinary 1x1 conv behind / in front of a probed one: (op, wq, w_scale, bias)"""
    N, C, H, W = shape_in
    wq = rng.integers(-127, 128, (K, C, 1, 1)).astype(np.int8)
    ws = np.full(K, 1.0 / 1024, np.float32)
    b = (rng.standard_normal(K) * 0.5).astype(np.float32)
    op = S.SaberConv2D(int8=True).init((N, C, H, W), S.ConvParam(wq, b, 1, (0, 0), (1, 1), (1, 1), bool(relu), ws), idt, odt, in_scale, out_scale)
    return op, wq, ws, b


@pytest.mark.parametrize("case", CHAIN_CASES)
def test_conv1x1_chain_first_epilogue_probes(case):
    """[1x1 conv + fused eltwise] -> 1x1 conv in one launch (chain_elt_pack): the first epilogue through y1 with every coefficient
    set (three of them with c0 != c1), s8 and u8 input; the second conv reads y1, so its output is checked against the oracle too."""
    Cc, HW, tn = case
    geo = (1, HW, HW, Cc, 4 * Cc, 1, 0, 1)
    rng = np.random.default_rng(Cc + HW)
    runs, n_new = 0, 0
    for idt, relu, res_relu, mode in P.ELT_COMBOS:
        if relu:
            continue                                   # (the chain's first conv has no relu of its own)
        n_new += mode in P.COEFF_MODES
        p = P.build("elt/chain/%s/relu%d_res%d/%s" % (P.DT_NAME[idt], relu, res_relu, mode), geo)
        P.assert_classes(p)
        want1 = P.oracle_bytes(p)
        ca = make_conv(p)
        s_sum = 1.0
        cb, wq2, ws2, b2 = _random_conv(rng, (1, 4 * Cc, HW, HW), Cc, P.S8, P.U8, 1, s_sum, float(P.U_SCALE))
        bp2, sc2 = O.conv_i8_prepare(ws2, b2, s_sum, float(P.U_SCALE), O.S8, O.U8)
        want2 = O.conv_i8(want1, wq2, bp2, sc2, O.U8, 1)
        chain = S.SaberConvChain(ca, cb)
        if tn is not None:
            chain.set_tile(tn)
        z1, z2 = ca.new_output(), cb.new_output()
        z1.fill_(SENTINEL)
        z2.fill_(SENTINEL)
        chain.dispatch(dev(p.x), dev(p.elt[0]), z1, z2)
        assert tn is None or chain.tile() == tn
        check(p, host(z1), want1, "chain y1, tile %s" % chain.tile())
        check(None, host(z2), want2, "chain y2, tile %s" % chain.tile())
        runs += 1
    assert runs == 4 * len(P.ELT_MODES) and n_new == 12, (runs, n_new)
    print("chain C=%d %dx%d tile %s: %d elt probes, %d of them with c0 != c1" % (Cc, HW, HW, tn, runs, n_new))


@pytest.mark.parametrize("case", CHAIN_CASES)
def test_conv1x1_chain_second_epilogue_probes(case):
    """The chain's second epilogue (chain_out_pack): the first conv is zeroed (weights and bias 0, c * s_res = 1), so y1 == res and res
    carries the probe's controlled bytes; s8 and u8 output, relu on and off."""
    Cc, HW, tn = case
    geo2 = (1, HW, HW, 4 * Cc, Cc, 1, 0, 1)
    runs = 0
    for odt in (P.S8, P.U8):
        for relu in (0, 1):
            p = P.build("conv/chain2/s8%s/relu%d" % (P.DT_NAME[odt], relu), geo2)
            P.assert_classes(p)
            want2 = P.oracle_bytes(p)
            cp = S.ConvParam(np.zeros((4 * Cc, Cc, 1, 1), np.int8), np.zeros(4 * Cc, np.float32), 1, (0, 0), (1, 1), (1, 1), False,
                             np.full(4 * Cc, 0.5, np.float32))
            cp.res_mode, cp.res_relu, cp.sum_scale, cp.coeff, cp.scale_res = L.RES_ELTWISE, False, 1.0, (1.0, 1.0), 1.0
            ca = S.SaberConv2D(int8=True).init((1, Cc, HW, HW), cp, P.U8, P.S8, 1.0, 1.0)
            cb = make_conv(p)
            chain = S.SaberConvChain(ca, cb)
            if tn is not None:
                chain.set_tile(tn)
            z1, z2 = ca.new_output(), cb.new_output()
            z1.fill_(SENTINEL)
            z2.fill_(SENTINEL)
            x0 = np.random.default_rng(HW).integers(0, 256, (1, HW, HW, Cc)).astype(np.uint8)
            chain.dispatch(dev(x0), dev(p.x), z1, z2)
            check(None, host(z1), p.x, "chain y1 == res, tile %s" % chain.tile())
            check(p, host(z2), want2, "chain y2, tile %s" % chain.tile())
            runs += 1
    print("chain second epilogue C=%d %dx%d tile %s: %d probes" % (Cc, HW, HW, tn, runs))


# ---- 3x3-led chains and the persistent stage ---------------------------------------------------------------------------------------------
# A fused launch keeps its intermediate tensors to itself, so each of its three epilogues is probed with the other two convs made
# transparent: a pass-through conv has one unit weight per output channel (input channel k % C, the centre tap) and scale exactly 1, a
# zeroed conv + eltwise with c * s_res = 1 hands its residual on unchanged.
def _passthrough(N, H, W, C, K, k, idt, odt, relu=False, elt=False, shift=0.0):
    """(op, f): y = f(x) = sat(x[..., k % C] + shift) channel by channel; with elt, a fused eltwise that adds a zero residual"""
    wq = np.zeros((K, C, k, k), np.int8)
    wq[np.arange(K), np.arange(K) % C, k // 2, k // 2] = 1
    cp = S.ConvParam(wq, np.full(K, shift, np.float32), 1, (k // 2, k // 2), (1, 1), (1, 1), bool(relu), np.ones(K, np.float32))
    if elt:
        cp.res_mode, cp.res_relu, cp.sum_scale, cp.coeff, cp.scale_res = L.RES_ELTWISE, False, 1.0, (1.0, 1.0), 1.0
    s_i, s_o = P._io_scales(idt, odt)
    op = S.SaberConv2D(int8=True).init((N, C, H, W), cp, idt, odt, s_i, s_o)
    lo, hi = P.RANGE[odt]

    def f(x):
        v = x.astype(np.int64)[..., np.arange(K) % C] + int(shift)
        return np.clip(np.maximum(v, 0) if relu else v, lo, hi).astype(P.NP_DT[odt])
    return op, f


def _zeroed_elt(N, H, W, C, K, idt):
    """1x1 conv with zero weights and bias + eltwise with c * s = 1: its output is its residual"""
    cp = S.ConvParam(np.zeros((K, C, 1, 1), np.int8), np.zeros(K, np.float32), 1, (0, 0), (1, 1), (1, 1), False, np.full(K, 0.5, np.float32))
    cp.res_mode, cp.res_relu, cp.sum_scale, cp.coeff, cp.scale_res = L.RES_ELTWISE, False, 1.0, (1.0, 1.0), 1.0
    return S.SaberConv2D(int8=True).init((N, C, H, W), cp, idt, P.S8, P._io_scales(idt, P.S8)[0], 1.0)


def _oracle_1x1(x, wq, ws, b, in_scale, out_scale, odt, relu):
    bp, sc = O.conv_i8_prepare(ws, b, in_scale, out_scale, O.code_of(x), odt)
    return O.conv_i8(x, wq, bp, sc, odt, relu)


class _Block:
    """one [3x3 -> 1x1 + eltwise -> 1x1] block with ONE probed conv (which = 0, 1, 2) and the other two transparent or ordinary"""

    def __init__(self, which, probe_name, N, H, W, C, idt, mdt, odt2, relu2, rng, x=None, res=None):
        K1 = 4 * C
        self.which, self.x, self.res = which, x, res
        relu0 = mdt == P.U8
        if which == 0:      # the 3x3's own requantisation, seen through a pass-through 1x1 (+ eltwise with a zero residual)
            self.p = P.build(probe_name % (P.DT_NAME[idt] + P.DT_NAME[mdt], int(relu0)), (N, H, W, C, C, 3, 1, 1))
            self.c0 = make_conv(self.p)
            self.ca, f = _passthrough(N, H, W, C, K1, 1, mdt, P.S8, elt=True, shift=-128.0 if mdt == P.U8 else 0.0)
            self.x = self.p.x
            self.res = np.zeros((N, H, W, K1), np.int8)
            self.want1 = f(P.oracle_bytes(self.p))
            self.src = lambda i: (i[0], i[1], i[2], i[3] % C)
        elif which == 1:    # the fused eltwise of the first 1x1: the 3x3 passes the probe's input through
            self.p = P.build(probe_name % P.DT_NAME[mdt], (N, H, W, C, K1, 1, 0, 1))
            self.c0, f = _passthrough(N, H, W, C, C, 3, mdt, mdt, relu=relu0)
            self.ca = make_conv(self.p)
            self.x, self.res = self.p.x, self.p.elt[0]
            assert np.array_equal(f(self.x), self.x)
            self.want1 = P.oracle_bytes(self.p)
            self.src = lambda i: i
        else:               # the last 1x1's epilogue: the first 1x1 is zeroed, its residual carries the probe's input
            self.p = P.build(probe_name % ("s8" + P.DT_NAME[odt2], relu2), (N, H, W, K1, C, 1, 0, 1))
            self.c0, f = _passthrough(N, H, W, C, C, 3, idt, mdt, relu=relu0)
            self.ca = _zeroed_elt(N, H, W, C, K1, mdt)
            if self.x is None:
                self.x = (rng.integers(0, 256, (N, H, W, C)).astype(np.uint8) if idt == P.U8 else rng.integers(-128, 128, (N, H, W, C)).astype(np.int8))
            self.res = self.p.x
            self.want1 = self.p.x
            self.src = None
        if which == 2:
            self.cb = make_conv(self.p)
            self.want2 = P.oracle_bytes(self.p)
        else:
            self.cb, wq2, ws2, b2 = _random_conv(rng, (N, K1, H, W), C, P.S8, odt2, relu2, 1.0, P._io_scales(P.S8, odt2)[1])
            self.want2 = _oracle_1x1(self.want1, wq2, ws2, b2, 1.0, P._io_scales(P.S8, odt2)[1], odt2, relu2)
        P.assert_classes(self.p)

    def check(self, z1, z2, what):
        if self.which == 2:
            check(None, z1, self.want1, what + " y1 (= the residual)")
            check(self.p, z2, self.want2, what + " y2")
            return
        if not np.array_equal(z1, self.want1):
            i = tuple(int(v) for v in np.argwhere(z1 != self.want1)[0])
            raise AssertionError("%s: %s y1: %d bytes differ, first at %s: got %d, want %d (%s)" % (
                self.p.name, what, int((z1 != self.want1).sum()), i, int(z1[i]), int(self.want1[i]), P.describe(self.p, self.src(i))))
        check(None, z2, self.want2, what + " y2")


CHAIN3_CASES = [(64, 7, 9, None), (128, 5, 17, None), (128, 5, 17, 5), (128, 5, 17, 6), (256, 3, 5, None), (256, 3, 5, 3), (256, 3, 5, 7),
                (256, 3, 5, 15)]      # C, H, W, tile code: the smallest shape per channel count of tests/test_gpu_parity.py's CHAIN3_CASES
_BLOCK_PROBES = [(0, "conv/chain3/%s/relu%d", (P.U8, P.U8)), (0, "conv/chain3/%s/relu%d", (P.S8, P.S8)), (0, "conv/chain3/%s/relu%d", (P.U8, P.S8)),
                 (0, "conv/chain3/%s/relu%d", (P.S8, P.U8))] + \
                [(1, "elt/chain3/%%s/relu0_res%d/%s" % (rr, m), (dt, dt)) for dt in (P.U8, P.S8) for rr in (0, 1) for m in P.ELT_MODES] + \
                [(2, "conv/chain3b/%s/relu%d", (P.U8, P.U8)), (2, "conv/chain3b/%s/relu%d", (P.S8, P.S8))]


@pytest.mark.parametrize("case", CHAIN3_CASES)
def test_conv3x3_chain_probes_each_of_its_three_epilogues(case):
    """3x3 conv -> [1x1 conv + eltwise] -> 1x1 conv in one launch (conv1x1_chain.hip, conv_chain_coop.hip), with and without the last conv:
    the 3x3's internal requantisation through a pass-through 1x1, the fused eltwise with every coefficient set, the last epilogue with
    the first 1x1 zeroed. The cooperative forms (tile codes 7, 15) run three launches: their arrival counters are never reset."""
    Cc, H, Wd, tn = case
    rng = np.random.default_rng(Cc + H)
    runs, n_elt, n_new = 0, 0, 0
    for which, name, (idt, mdt) in _BLOCK_PROBES:
        for odt2, relu2 in ((P.U8, 1), (P.S8, 0)):
            if which != 2 and odt2 == P.S8:
                continue
            n_elt += which == 1
            n_new += which == 1 and name.rsplit("/", 1)[1] in P.COEFF_MODES
            b = _Block(which, name, 1, H, Wd, Cc, idt, mdt, odt2, relu2, rng)
            chain = S.SaberConvChain(b.ca, b.cb, conv3x3=b.c0)
            if tn is not None:
                chain.set_tile(tn)
            xd, rd = dev(b.x), dev(b.res)
            z1, z2 = b.ca.new_output(), b.cb.new_output()
            for rep in range(3 if tn in (7, 15) else 1):
                z1.fill_(SENTINEL)
                z2.fill_(SENTINEL)
                chain.dispatch(xd, rd, z1, z2)
                assert tn is None or chain.tile() == tn
                b.check(host(z1), host(z2), "chain tile %s launch %d" % (chain.tile(), rep))
            if which != 2:
                double = S.SaberConvChain(b.ca, None, conv3x3=b.c0)
                if tn is not None and tn not in (7, 15):
                    double.set_tile(tn)
                z1.fill_(SENTINEL)
                double.dispatch(xd, rd, z1)
                b.check(host(z1), b.want2, "3x3 + 1x1 only, tile %s" % double.tile())
            runs += 1
    assert n_elt == 4 * len(P.ELT_MODES) and n_new == 12, (n_elt, n_new)
    print("chain3 C=%d %dx%d tile %s: %d probes, %d elt probes, %d of them with c0 != c1" % (Cc, H, Wd, tn, runs, n_elt, n_new))


@pytest.mark.parametrize("shape", P.STAGE_PROBE_SHAPES)
def test_chain_stage_probes_each_epilogue_of_its_first_block(shape):
    """Two blocks in one persistent launch (conv_stage_coop.hip; C = 256, 128 and 64 - conv_stage1_c64_kernel on two column tiles with a
    ragged one, four and three tile rows with a ragged last one, two images): block 1 carries the probe in one of its three convs, block 2 reads block
    1's two outputs through pass-through convs, so its outputs show the bytes that crossed the edge barrier. Three launches each."""
    Cc, N, H, Wd = shape
    rng = np.random.default_rng(Cc + N)
    runs, n_elt, n_new = 0, 0, 0
    for which, name, (idt, mdt) in _BLOCK_PROBES:
        if mdt != P.U8:
            continue                                   # (a stage's 3x3 convs write u8, as the network's do)
        n_elt += which == 1
        n_new += which == 1 and name.rsplit("/", 1)[1] in P.COEFF_MODES
        b1 = _Block(which, name, N, H, Wd, Cc, idt, mdt, P.U8, 1, rng)
        # block 2: 3x3 pass-through of block 1's y2 (u8), 1x1 pass-through - 128 + eltwise adding block 1's y1, an ordinary last conv
        K1 = 4 * Cc
        c0, f0 = _passthrough(N, H, Wd, Cc, Cc, 3, P.U8, P.U8, relu=True)
        ca, f1 = _passthrough(N, H, Wd, Cc, K1, 1, P.U8, P.S8, elt=True, shift=-128.0)
        cb, wq2, ws2, b2 = _random_conv(rng, (N, K1, H, Wd), Cc, P.S8, P.U8, 1, 1.0, float(P.U_SCALE))
        q = f1(f0(b1.want2)).astype(np.int64) + b1.want1.astype(np.int64)          # c * s = 1: t = q + r, an integer
        want1 = np.clip(q, -128, 127).astype(np.int8)
        want2 = _oracle_1x1(want1, wq2, ws2, b2, 1.0, float(P.U_SCALE), O.U8, 1)
        chains = [S.SaberConvChain(b1.ca, b1.cb, conv3x3=b1.c0), S.SaberConvChain(ca, cb, conv3x3=c0)]
        stage = S.SaberChainStage(chains)
        y1 = [b1.ca.new_output(), ca.new_output()]
        y2 = [b1.cb.new_output(), cb.new_output()]
        xd, rd = dev(b1.x), dev(b1.res)
        for rep in range(3):
            for t in y1 + y2:
                t.fill_(SENTINEL)
            stage.dispatch(xd, rd, y1, y2)
            b1.check(host(y1[0]), host(y2[0]), "stage block 1, launch %d" % rep)
            check(None, host(y1[1]), want1, "stage block 2 y1 (block 1's outputs passed through), launch %d, probe %s" % (rep, b1.p.name))
            check(None, host(y2[1]), want2, "stage block 2 y2, launch %d, probe %s" % (rep, b1.p.name))
        runs += 1
    assert runs == len(P.stage_block_probes(shape)) and n_elt == 2 * len(P.ELT_MODES) and n_new == 6, (runs, n_elt, n_new)
    print("stage C=%d N=%d %dx%d: %d probes x 3 launches, %d elt probes, %d of them with c0 != c1" % (Cc, N, H, Wd, runs, n_elt, n_new))


# ---- the streaming ops -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", sorted(P.ELT_SETS))
def test_eltwise_sum_s8_every_pair_of_bytes(mode):
    """SaberEltwise<AK_INT8> sum on ALL 65536 (a, b) pairs per coefficient set, relu on and off: ties go half away, both rails, the
    association (c * a) * s, t = +-0x1.fffffep-2 (the roundf identity's edge), and three sets with c0 != c1."""
    c, s0, s1 = P.ELT_SETS[mode]
    a, b = P.eltwise_grid()
    for relu in (False, True):
        want = O.eltwise_i8(a, b, s0, s1, c[0], c[1], relu)
        got = host(S.eltwise_sum(dev(a), dev(b), c, relu, s0, s1))
        if not np.array_equal(got, want):
            i = tuple(int(v) for v in np.argwhere(got != want)[0])
            raise AssertionError("eltwise %s relu %d: %d bytes differ, first a %d b %d: got %d, oracle %d" %
                                 (mode, relu, int((got != want).sum()), int(a[i]), int(b[i]), int(got[i]), int(want[i])))


@pytest.mark.parametrize("odt", [P.S8, P.U8])
def test_quantize_ties_go_half_away_and_rails_saturate(odt):
    """quantize_nchw_to_nhwc (s8 and u8) and quantize_flat_s8: x / scale exactly m + 0.5 for both signs and parities, +-0x1.fffffep-2,
    the values one ulp beside a tie, both rails, +-1e6."""
    x, scale = P.quant_values(odt)
    want = O.quant_nchw_to_nhwc(x, scale, odt)
    assert np.array_equal(want, P.quant_model(x, odt).transpose(0, 2, 3, 1))
    got = host(S.quantize_nchw_to_nhwc(dev(x), scale, odt))
    bad = np.argwhere(got != want)
    assert len(bad) == 0, ("quantize_nchw_to_nhwc", P.DT_NAME[odt], len(bad), bad[0], float(x.transpose(0, 2, 3, 1)[tuple(bad[0])]),
                           int(got[tuple(bad[0])]), int(want[tuple(bad[0])]))
    if odt == P.S8:
        flat = x.reshape(4, -1)
        wantf = O.quant_flat_s8(flat, 1.0)
        gotf = host(S.quantize_flat_s8(dev(flat), 1.0))
        bad = np.argwhere(gotf != wantf)
        assert len(bad) == 0, ("quantize_flat_s8", len(bad), bad[0], float(flat[tuple(bad[0])]), int(gotf[tuple(bad[0])]), int(wantf[tuple(bad[0])]))


@pytest.mark.parametrize("dt", [P.S8, P.U8])
def test_average_pooling_i8_window_sums_on_exact_halves(dt):
    """Average and global-average pooling_i8 round sum * (1 / count) half-even: a checkerboard of (a, b) with a + b odd makes every window
    with an even cell count sum to count * (m + 0.5) - windows 2x2, 3x3 and 7x7 (whole and clipped at the border), global on 8x8, 4x4, 7x7."""
    x = P.pool_image(dt)
    for win, st, pad, pt in P.POOL_WINDOWS:
        want = O.pool_i8_nhwc(x, win, st, pad, pt)
        assert np.array_equal(want, P.pool_model(x, win, st, pad, pt, want.shape[1:3]))
        got = host(S.pooling_i8(dev(x), win, st, pad, pt))
        bad = np.argwhere(got != want)
        assert len(bad) == 0, ("pooling_i8", win, st, pad, pt, len(bad), bad[0], int(got[tuple(bad[0])]), int(want[tuple(bad[0])]))
    for hw in ((8, 8), (4, 4), (7, 7), (2, 3)):
        xg = P.pool_image(dt, *hw)
        want = O.pool_i8_nhwc(xg, None, None, None, 1, global_pool=True)
        assert np.array_equal(want, P.pool_model(xg, None, None, None, 1, None, global_pool=True))
        got = host(S.pooling_i8(dev(xg), None, None, None, 1, global_pooling=True))
        bad = np.argwhere(got != want)
        assert len(bad) == 0, ("global pooling_i8", hw, len(bad), bad[0], int(got[tuple(bad[0])]), int(want[tuple(bad[0])]))


@pytest.mark.parametrize("M", [1, 8])
@pytest.mark.parametrize("idt", [P.S8, P.U8])
def test_fc_i8_controlled_accumulators(M, idt):
    """SaberFc INT8 (K = 512, N = 24): chosen accumulators, scales and biases with full mantissas - (float)acc * scale + bias in two
    roundings (s8 operand) resp. scale * (float)(acc + (int)(bias / scale)) (u8); the logits of dispatch_softmax are the same bits."""
    K, N = 512, 24
    x, wq, ws, b, s_in, s_out = P.fc_probe(M, K, N, idt)
    fc = S.SaberFc(True).init(M, N, K, wq, b, idt, s_in, s_out, w_scale=ws)
    assert fc.algo() == "fc_i8_small_16xk4", fc.algo()
    want = O.fc_i8(x, wq, ws, s_in, b, s_out) if idt == P.U8 else O.fc_i8(x, wq, ws, s_in, b)
    y = torch.full((M, N), -7.0, dtype=torch.float32, device="cuda")
    prob = torch.full((M, N), -1.0, dtype=torch.float32, device="cuda")
    got = host(fc.dispatch(dev(x), y))
    assert np.array_equal(got, want), (np.argwhere(got != want)[0], got[got != want][:4], want[got != want][:4])
    y.fill_(-7.0)
    fc.dispatch_softmax(dev(x), y, prob)
    assert np.array_equal(host(y), want)
    sm = O.softmax_f32(want)
    assert np.abs(host(prob) - sm).max() <= 1e-4 * sm.max()


# ---- stem conv + max pooling, stem pair --------------------------------------------------------------------------------------------------
def _stem_pool_op(p, f32_in):
    N, H, W, C, K, k, pad, stride = p.geo
    cp = S.ConvParam(p.wq, p.bias, 1, (3, 3), (2, 2), (1, 1), p.relu, p.w_scale)
    op = S.SaberConv2DPooling().init((N, 3, H, W), cp, L.POOL_MAX, (3, 3), (2, 2), (0, 0), L.F32 if f32_in else p.idt, p.odt, p.in_scale,
                                     p.out_scale, in_layout=L.NCHW if f32_in else L.NHWC)
    assert op.fused and "maxpool" in op.algo(), op.algo()
    return op


def _check_pooled(p, got, want, what):
    if np.array_equal(got, want):
        return
    i = tuple(int(v) for v in np.argwhere(got != want)[0])
    raise AssertionError("%s: %s: %d pooled bytes differ, first at %s: got %d, oracle %d (centre output: %s)" % (
        p.name, what, int((got != want).sum()), i, int(got[i]), int(want[i]), P.describe(p, (i[0], 2 * i[1] + 1, 2 * i[2] + 1, i[3]))))


@pytest.mark.parametrize("group", sorted(g for g in GROUPS if g.startswith("stempool/")))
def test_stem_conv_maxpool_probes(group):
    """SaberConv2DPooling (7x7 / 2 stem + 3x3 / 2 max pooling in one launch, its own epilogue in conv_stem.h): the probed outputs sit on
    the pooling windows' centres over the smallest / largest background, so each class survives its window. u8 / s8 NHWC input, and the
    s8 probe again as an f32 NCHW image whose quantise-on-entry step meets exact ties (it rounds half away)."""
    names = GROUPS[group]
    for a, b in zip(names[0::2], names[1::2]):
        P.assert_classes(P.build(a), P.build(b))
    runs = 0
    for name in names:
        p = P.build(name)
        want = P.max_pool_3x3s2(P.oracle_bytes(p))
        for f32_in in ((False, True) if p.idt == P.S8 else (False,)):
            op = _stem_pool_op(p, f32_in)
            y = op.new_output()
            y.fill_(SENTINEL)
            op.dispatch(dev(P.f32_image_of(p.x) if f32_in else p.x), y)
            _check_pooled(p, host(y), want, "%s%s" % (op.algo(), " f32 image" if f32_in else ""))
            runs += 1
    print("%s: %d launches" % (group, runs))


@pytest.mark.parametrize("hw", P.STEM_POOL_IMAGES)
@pytest.mark.parametrize("f32_in", [False, True])
def test_stem_pair_probes_the_stem_epilogue(hw, f32_in):
    """SaberStemPair: stem + pooling + the two 1x1 convs reading the pooled tensor in one launch; the stem carries the probe (its pooled
    tensor is written on request and checked), the two convs behind it are ordinary ones checked against the oracle. s8 and u8 NHWC
    images and the f32 NCHW image."""
    rng = np.random.default_rng(hw[0])
    for odt, bg, idt in [(o, g, i) for o in (P.U8, P.S8) for g in ("bgmin", "bgmax") for i in ((P.S8,) if f32_in else (P.S8, P.U8))]:
        p = P.build("conv/stempool%dx%d/%s%s/relu%d/%s" % (hw + (P.DT_NAME[idt], P.DT_NAME[odt], odt == P.U8, bg)))
        pooled = P.max_pool_3x3s2(P.oracle_bytes(p))
        stem = _stem_pool_op(p, f32_in)
        N, ph, pw, _ = pooled.shape
        convs, wants = [], []
        for K, kdt, relu in ((256, P.S8, 0), (64, P.U8, 1)):
            s_i, s_o = P._io_scales(odt, kdt)
            op, wq, ws, b = _random_conv(rng, (N, 64, ph, pw), K, odt, kdt, relu, s_i, s_o)
            convs.append(op)
            wants.append(_oracle_1x1(pooled, wq, ws, b, s_i, s_o, kdt, relu))
        sp = S.SaberStemPair(stem, convs[0], convs[1])
        ya, yb, yp = convs[0].new_output(), convs[1].new_output(), stem.new_output()
        for t in (ya, yb, yp):
            t.fill_(SENTINEL)
        sp.dispatch(dev(P.f32_image_of(p.x) if f32_in else p.x), ya, yb, yp)
        _check_pooled(p, host(yp), pooled, "stem pair, pooled tensor")
        check(None, host(ya), wants[0], "stem pair first conv, probe %s" % p.name)
        check(None, host(yb), wants[1], "stem pair second conv, probe %s" % p.name)


# ---- fused global average pooling on the image-resident 1x1 ------------------------------------------------------------------------------
def test_image_resident_conv_with_fused_global_pooling_probes():
    """set_global_pooling: the conv's bytes and rne(sum over the pixels * (1 / 16)) of them in one launch (stage_xcd.hip); 4x4 pixels,
    bias' found by search so that the channels' byte sums are exact ties of the pooled value."""
    runs, ties = 0, 0
    for name in P.GPOOL_NAMES:
        p = P.build(name)
        want = P.oracle_bytes(p)
        want_pool = O.pool_i8_nhwc(want, None, None, None, 1, global_pool=True)
        n_tie = int((want.astype(np.int64).sum(axis=(1, 2)) % 16 == 8).sum())
        assert n_tie >= 4, (name, n_tie)
        ties += n_tie
        conv = make_conv(p)
        conv.set_tile(12 << 16)
        conv.set_global_pooling()
        assert conv.algo().endswith("+gpool"), conv.algo()
        y = conv.new_output()
        yp = torch.full(want_pool.shape, SENTINEL, dtype=y.dtype, device="cuda")
        y.fill_(SENTINEL)
        conv.dispatch_gpool(dev(p.x), y, yp)
        check(p, host(y), want, conv.algo())
        check(None, host(yp), want_pool, conv.algo() + " pooled, probe " + name)
        runs += 1
    print("gpool: %d launches, %d pooled sums on an exact tie" % (runs, ties))


# ---- the strided-head chain, depthwise -------------------------------------------------------------------------------------------------
def test_strided_head_chain_probes():
    """3x3 / stride 2 -> [1x1 + eltwise on the sub-sampled shortcut] in one launch (C = 64, 9x7 -> 5x4): the 3x3's requantisation through
    a pass-through 1x1, then the fused eltwise (every coefficient set) behind a pass-through 3x3."""
    N, H, Wd, Cc, K1 = 1, 9, 7, 64, 256
    Ho, Wo = 5, 4
    runs = 0
    for relu_name, mdt in (("u8u8/relu1", P.U8),):
        p = P.build("conv/head/" + relu_name, (N, H, Wd, Cc, Cc, 3, 1, 2))
        P.assert_classes(p)
        c0 = make_conv(p)
        shift = -128 if mdt == P.U8 else 0
        wq = np.zeros((K1, Cc, 1, 1), np.int8)
        wq[np.arange(K1), np.arange(K1) % Cc, 0, 0] = 1
        cp = S.ConvParam(wq, np.full(K1, shift, np.float32), 1, (0, 0), (1, 1), (1, 1), False, np.ones(K1, np.float32))
        cp.res_mode, cp.res_relu, cp.sum_scale, cp.coeff, cp.scale_res = L.RES_ELTWISE, False, 1.0, (1.0, 1.0), 1.0
        cp.res_stride, cp.res_hw = 2, (H, Wd)
        ca = S.SaberConv2D(int8=True).init((N, Cc, Ho, Wo), cp, mdt, P.S8, P._io_scales(mdt, P.S8)[0], 1.0)
        want = (P.oracle_bytes(p).astype(np.int64)[..., np.arange(K1) % Cc] + shift).astype(np.int8)
        chain = S.SaberConvChain(ca, None, conv3x3=c0)
        z1 = ca.new_output()
        z1.fill_(SENTINEL)
        chain.dispatch(dev(p.x), dev(np.zeros((N, H, Wd, K1), np.int8)), z1)
        got = host(z1)
        if not np.array_equal(got, want):
            i = tuple(int(v) for v in np.argwhere(got != want)[0])
            raise AssertionError("%s: strided head: first bad %s got %d want %d (%s)" % (p.name, i, int(got[i]), int(want[i]),
                                                                                         P.describe(p, (i[0], i[1], i[2], i[3] % Cc))))
        runs += 1
    for res_relu in (0, 1):
        for mode in P.ELT_MODES:
            p = P.build("elt/head/u8/relu0_res%d/%s" % (res_relu, mode), (N, Ho, Wo, Cc, K1, 1, 0, 1))
            P.assert_classes(p)
            x = np.zeros((N, H, Wd, Cc), np.uint8)
            x[:, ::2, ::2] = p.x
            res = np.full((N, H, Wd, K1), SENTINEL, np.int8)
            res[:, ::2, ::2] = p.elt[0]
            wq = np.zeros((Cc, Cc, 3, 3), np.int8)
            wq[np.arange(Cc), np.arange(Cc), 1, 1] = 1
            c0 = S.SaberConv2D(int8=True).init((N, Cc, H, Wd), S.ConvParam(wq, None, 1, (1, 1), (2, 2), (1, 1), True, np.ones(Cc, np.float32)),
                                               P.U8, P.U8, float(P.U_SCALE), float(P.U_SCALE))
            N_, H_, W_, C_, K_, k_, pad_, st_ = p.geo
            cp = S.ConvParam(p.wq, p.bias, 1, (0, 0), (1, 1), (1, 1), False, p.w_scale)
            cp.res_mode, cp.res_relu, cp.sum_scale, cp.coeff, cp.scale_res = L.RES_ELTWISE, p.elt[1], 1.0, p.elt[2], p.elt[3]
            cp.res_stride, cp.res_hw = 2, (H, Wd)
            ca = S.SaberConv2D(int8=True).init((N, Cc, Ho, Wo), cp, P.U8, P.S8, p.in_scale, p.out_scale)
            chain = S.SaberConvChain(ca, None, conv3x3=c0)
            z1 = ca.new_output()
            z1.fill_(SENTINEL)
            chain.dispatch(dev(x), dev(res), z1)
            check(p, host(z1), P.oracle_bytes(p), "strided head, eltwise")
            runs += 1
    assert runs == 1 + 2 * len(P.ELT_MODES)
    print("strided head: %d probes, %d elt probes, %d of them with c0 != c1" % (runs, runs - 1, 2 * len(P.COEFF_MODES)))


@pytest.mark.parametrize("group", sorted(g for g in GROUPS if g.startswith("dw/")))
def test_depthwise_probes_every_form(group):
    """Depthwise 3x3 (selection variant 16), stride 1 and 2: the static choice, the direct kernel (form 0) and every depthwise form, all
    four dtype combinations, relu on and off."""
    from tests import dw_util as DU
    seen = set()
    for name in GROUPS[group]:
        p = P.build(name)
        P.assert_classes(p)
        N, H, W, C, K, k, pad, stride = p.geo
        cp = S.ConvParam(p.wq, p.bias, C, (pad, pad), (stride, stride), (1, 1), p.relu, p.w_scale)
        conv = S.SaberConv2D(True).init((N, C, H, W), cp, p.idt, p.odt, p.in_scale, p.out_scale, in_layout=L.NHWC, out_layout=L.NHWC)
        lib = L.load()
        assert lib.saber_hip_conv2d_get_tile(conv.h) >> 16 == 16, conv.algo()
        forms = DU.dw_forms(lib, conv.h)
        assert len(forms) >= 2, forms
        want = P.oracle_bytes(p)
        xd = dev(p.x)
        for code in [None, 16 << 16] + [(16 << 16) | v for v in forms]:
            if code is not None:
                conv.set_tile(code)
            y = conv.new_output()
            y.fill_(SENTINEL)
            conv.dispatch(xd, y)
            check(p, host(y), want, "%s (%s)" % (conv.algo(), code))
            seen.add(conv.algo())
    assert "direct_i8" in seen and sum(a.startswith("dw3x3_i8_") for a in seen) >= 2, seen
    print("%s: %d probes, forms: %s" % (group, len(GROUPS[group]), " ".join(sorted(seen))))
