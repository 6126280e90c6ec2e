"""saber_hip_conv2d_set_weights / saber_hip_fc_set_weights on LIVE ops: the cases tests/test_gpu_live_weights.py runs, their oracle results and
the outputs of the STALE MODELS - what an op would compute that kept exactly one ingredient of its first parameter set - so that
tests/test_live_weights_cpu.py can prove on the CPU that each of them is told from the right answer. Plain numpy plus the CPU oracle, no device.
TEST INFRASTRUCTURE ONLY.

A case = a geometry, an input of the op's dtype and two parameter sets A and B: weights and bias are independent random draws, B's in_scale and
out_scale are A's times 1.37 and 0.73 (no powers of two: a stale scale changes mantissas, not only exponents).

  stale models (B with ONE ingredient left at A, as the tables set_weights uploads):
    weights     the quantised weights
    bias        the bias' table (bias / (w_scale * in_scale))
    in_scale    in_scale inside bias' and the per-channel scale
    out_scale   out_scale inside the per-channel scale (8-bit outputs)
    comp        u8 input: the 128 * sum(w) compensation of the u8 -> s8 shift - acc + 128 * (sum(wq_A) - sum(wq_B)) per channel
    scale_conv  fused eltwise: the eltwise's first scale alone
    reverse     fused eltwise: everything A, scale_conv B (what a composite computes that reads its member's CURRENT out_scale beside its own
                copy of the member's packing)
  model() is the float32 numpy restatement of the oracle's epilogue (tests/int8_probe.py's helpers) that takes those ingredients one by one;
  the CPU test holds it to the oracle on A and B before it trusts it on the mixes.

A composite = a small graph of member convs; Composite.eval(pick) walks it with the oracle, member by member, under any choice of A / B per
member; Composite.documented(updated) is the choice include/saber_hip.h documents after set_weights(B) on the members in `updated`: a COPIED
member stays at A, a LIVE member follows."""
import numpy as np

from oracle import oracle as O
from tests import int8_probe as P

F = np.float32
F32, S8, U8 = O.F32, O.S8, O.U8
NP_DT = {F32: np.float32, S8: np.int8, U8: np.uint8}
IN_FACTOR, OUT_FACTOR = 1.37, 0.73
MIN_SHARE = 0.25
S_SUM = 0.06                                   # the scale of a fused eltwise's output: its coefficients are multiples of 1 / S_SUM
UNEQ = (1.0, -0.5)


def coeff_pair(mult, s_sum=S_SUM):
    c = 1.0 / s_sum
    return (float(F(mult[0] * c)), float(F(mult[1] * c)))


def rand8(rng, shape, dt):
    return (rng.integers(0, 256, shape) if dt == U8 else rng.integers(-128, 128, shape)).astype(NP_DT[dt])


def share(a, b):
    """the share of the output BYTES that differ"""
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    return float(np.mean(np.ascontiguousarray(a).view(np.uint8) != np.ascontiguousarray(b).view(np.uint8)))


class Spec:
    """one conv op: geo = (N, H, W, C, K, k, pad, stride); mode "conv" | "elt" (RES_ELTWISE, s8 out) | "sum" (RES_SUM_INPLACE); pool: the
    stem's fused 3x3 / 2 max pooling behind it"""

    def __init__(self, geo, idt, odt, relu, mode="conv", group=1, coeff=(1.0, 1.0), scale_res=1.0, res_relu=False, sum_scale=1.0, res_stride=0,
                 res_hw=(0, 0), pool=False):
        self.geo, self.idt, self.odt, self.relu, self.mode, self.group = tuple(geo), idt, odt, int(bool(relu)), mode, group
        self.coeff, self.scale_res, self.res_relu, self.sum_scale = coeff, scale_res, bool(res_relu), sum_scale
        self.res_stride, self.res_hw, self.pool = res_stride, res_hw, pool
        assert mode == "conv" or (mode == "elt" and odt == S8) or (mode == "sum" and odt != F32)

    @property
    def wshape(self):
        N, H, W, C, K, k, pad, stride = self.geo
        return (K, C // self.group, k, k)

    @property
    def pad(self):
        return (self.geo[6],) * 2

    @property
    def stride(self):
        return (self.geo[7],) * 2

    @property
    def conv_hw(self):
        N, H, W, C, K, k, pad, stride = self.geo
        return (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1


class Params:
    """one parameter set of one conv / fc: f32 weights, bias (or None), the two edge scales; the oracle's quantisation of the weights"""

    def __init__(self, w, bias, in_scale, out_scale):
        self.w, self.bias, self.in_scale, self.out_scale = w, bias, float(in_scale), float(out_scale)
        self.ws = O.weight_scales(w)
        self.wq = O.quant_weights(w, self.ws)

    def but(self, **kw):
        """a copy with other bias / scales (the weights and their quantisation shared)"""
        q = Params.__new__(Params)
        q.__dict__.update(self.__dict__)
        q.__dict__.update(kw)
        return q


def draw(rng, spec, in_scale, out_scale, bias=True):
    K, cg, k, _ = spec.wshape
    std = 0.4 if spec.group > 1 and cg == 1 else np.sqrt(2.0 / (cg * k * k))
    w = (rng.standard_normal(spec.wshape) * std).astype(F)
    b = (rng.standard_normal(K) * 0.5).astype(F) if bias else None
    return Params(w, b, in_scale, out_scale)


def draw_pair(rng, spec, in_scale, out_scale, bias=True):
    """(A, B): independent weights and bias, B's scales = A's x 1.37 / x 0.73"""
    return draw(rng, spec, in_scale, out_scale, bias), draw(rng, spec, in_scale * IN_FACTOR, out_scale * OUT_FACTOR, bias)


def _pool(y):
    return O.pool_i8_nhwc(y, (3, 3), (2, 2), (0, 0), 0)


def _sub(spec, res):
    s = spec.res_stride
    return O.pool_i8_nhwc(res, (1, 1), (s, s), (0, 0), 0, floor_mode=True) if s > 1 else res


def run(spec, x, p, res=None, prev=None):
    """the oracle's output of one op under parameter set p"""
    cdt = S8 if spec.mode == "elt" else spec.odt
    bp, sc = O.conv_i8_prepare(p.ws, p.bias, p.in_scale, p.out_scale, spec.idt, cdt)
    if spec.mode == "sum":
        rp = O.Residual(O.RES_JIT_SUM, 0, spec.sum_scale, spec.odt, 0, 0, 0, 0)
        return O.conv_i8(x, p.wq, bp, sc, spec.odt, spec.relu, spec.pad, spec.stride, residual=rp, out_init=prev)
    y = O.conv_i8(x, p.wq, bp, sc, cdt, spec.relu, spec.pad, spec.stride, group=spec.group)
    if spec.mode == "elt":
        y = O.eltwise_i8(y, _sub(spec, res), p.out_scale, spec.scale_res, spec.coeff[0], spec.coeff[1], spec.res_relu)
    return _pool(y) if spec.pool else y


# ---- the stale models ----------------------------------------------------------------------------------------------------------------------
def stale_kinds(spec):
    cdt = S8 if spec.mode == "elt" else spec.odt
    return ["weights", "bias", "in_scale"] + (["out_scale"] if cdt != F32 else []) + (["comp"] if spec.idt == U8 else []) + \
        (["scale_conv", "reverse"] if spec.mode == "elt" else [])


def ingredients(spec, A, B, stale=None):
    """what the epilogue is fed: B's tables with one of them left at A's"""
    cdt = S8 if spec.mode == "elt" else spec.odt

    def prep(p, in_scale=None, out_scale=None):
        return P.prepare(p.ws, p.bias, p.in_scale if in_scale is None else in_scale, p.out_scale if out_scale is None else out_scale, spec.idt, cdt)
    if stale == "reverse":
        bp, sc = prep(A)
        return dict(wq=A.wq, bp=bp, sc=sc, scale_conv=B.out_scale, acc_delta=0)
    bp, sc = prep(B)
    ing = dict(wq=B.wq, bp=bp, sc=sc, scale_conv=B.out_scale, acc_delta=0)
    if stale == "weights":
        ing["wq"] = A.wq
    elif stale == "bias":
        ing["bp"] = prep(A)[0]
    elif stale == "in_scale":
        ing["bp"], ing["sc"] = prep(B, in_scale=A.in_scale)
    elif stale == "out_scale":
        ing["sc"] = prep(B, out_scale=A.out_scale)[1]
    elif stale == "comp":
        ing["acc_delta"] = 128 * (A.wq.astype(np.int64).sum(axis=(1, 2, 3)) - B.wq.astype(np.int64).sum(axis=(1, 2, 3)))
    elif stale == "scale_conv":
        ing["scale_conv"] = A.out_scale
    else:
        assert stale is None, stale
    return ing


def model(spec, x, ing, res=None, prev=None):
    """the op's output by the float32 numpy model of the oracle's epilogue (tests/int8_probe.py: emulate), fed ingredient by ingredient"""
    assert spec.group == 1
    acc = P.int_conv(x, ing["wq"], spec.geo[6], spec.geo[7]) + ing["acc_delta"]
    d = P._conv_d(acc, ing["bp"], ing["sc"])
    if spec.mode == "sum":
        d = P._sum_d(d, prev, spec.sum_scale)
    if spec.relu or (spec.mode == "sum" and spec.odt == U8):
        d = np.maximum(d, F(0))
    if spec.mode == "elt":
        q = P._sat(P._round_conv(d), S8).astype(F)
        t = P._elt_t(q, _sub(spec, res), spec.coeff[0], spec.coeff[1], ing["scale_conv"], spec.scale_res)
        if spec.res_relu:
            t = np.maximum(t, F(0))
        y = P._sat(P._round_elt(t), S8)
    else:
        y = d.astype(F) if spec.odt == F32 else P._sat(P._round_conv(d), spec.odt)
    return _pool(y) if spec.pool else y


# ---- single ops ------------------------------------------------------------------------------------------------------------------------------
GEOMETRY_NAMES = ("pw_k64", "pw_k72", "pw_k34", "c3x3", "img3x3", "imgres1x1", "imgres3x3", "stem", "stempool18x23")
COMBOS = {"u8u8": (U8, U8, 1), "s8s8": (S8, S8, 0), "u8s8": (U8, S8, 1), "s8f32": (S8, F32, 0)}
S_IN, S_OUT, S_RES = 0.02, 0.05, 0.043
_cases = {}


def case_names(geometries=GEOMETRY_NAMES):
    """every single-op case: plain (the four dtype combinations; a fused pooling has no f32 output), and on P.FUSED_GEOMETRIES the fused
    eltwise with the unequal pair (1, -0.5) and the in-place sum"""
    out = []
    for g in geometries:
        out += ["%s/plain/%s" % (g, c) for c in COMBOS if not (g.startswith("stempool") and c == "s8f32")]
        if g in P.FUSED_GEOMETRIES:
            out += ["%s/elt/u8" % g, "%s/elt/s8" % g, "%s/sum/u8u8" % g, "%s/sum/s8s8" % g]
    return out


class Case:
    """one op, its input (and residual / the bytes already in y), parameter sets A and B, the oracle's outputs under both"""

    def __init__(self, name):
        g, epi, combo = name.split("/")
        geo = P.GEOMETRIES[g]
        seed = int.from_bytes(name.encode(), "little") % (2 ** 31)
        rng = np.random.default_rng(seed)
        pool = g.startswith("stempool")
        if epi == "plain":
            idt, odt, relu = COMBOS[combo]
            self.spec = Spec(geo, idt, odt, relu, pool=pool)
        elif epi == "elt":
            idt = U8 if combo == "u8" else S8
            self.spec = Spec(geo, idt, S8, 0, "elt", coeff=coeff_pair(UNEQ), scale_res=S_RES, res_relu=(idt == U8))
        else:
            idt, odt, relu = COMBOS[combo]
            self.spec = Spec(geo, idt, odt, relu, "sum", sum_scale=0.75)
        self.name = name
        N, H, W, C, K, k, pad, stride = geo
        oh, ow = self.spec.conv_hw
        self.x = rand8(rng, (N, H, W, C), self.spec.idt)
        self.res = rand8(rng, (N, oh, ow, K), S8) if epi == "elt" else None
        self.prev = rand8(rng, (N, oh, ow, K), self.spec.odt) if epi == "sum" else None
        # an input scale that keeps a good part of the outputs between the rails: |x| ~ 74 (s8) / 147 (u8) rms, He-scaled weights
        # (a max pooling keeps the largest of nine: a wider output scale keeps those off the rail)
        s_in = S_IN * (0.5 if idt == U8 else 1.0)
        self.A, self.B = draw_pair(rng, self.spec, s_in, S_OUT * (2.0 if pool else 1.0))
        self.want = {"A": run(self.spec, self.x, self.A, self.res, self.prev), "B": run(self.spec, self.x, self.B, self.res, self.prev)}
        self._stale = {}

    def stale(self, kind):
        if kind not in self._stale:
            self._stale[kind] = model(self.spec, self.x, ingredients(self.spec, self.A, self.B, kind), self.res, self.prev)
        return self._stale[kind]

    def model_of(self, which):
        """the numpy model on a whole parameter set (must equal want[which])"""
        p = self.A if which == "A" else self.B
        return model(self.spec, self.x, ingredients(self.spec, p, p), self.res, self.prev)


def case(name):
    if name not in _cases:
        _cases[name] = Case(name)
    return _cases[name]


# ---- fully connected -------------------------------------------------------------------------------------------------------------------------
FC_SHAPES = [(3, 40, 512), (8, 333, 1024)]            # (M, N, K)
FC_INPUTS = ("s8", "u8", "f32")                       # f32: an INT8 fc that quantises on entry (to s8)
_fc_cases = {}


class FcCase:
    """INT8 fc: x [M, K], two parameter sets (w [N, K] f32, bias, in_scale, out_scale - the u8 form's requantisation), the oracle's f32 outputs.
    Stale models through the oracle itself: O.fc_i8 takes every ingredient as an argument (a u8 fc keeps its bias INSIDE the compensation
    vector, so "comp" = the conv-style vector without the bias term, "bias" = comp made with A's bias)."""

    def __init__(self, shape, kind):
        M, N, K = shape
        rng = np.random.default_rng(90000 + 7 * M + N + K + 1000 * FC_INPUTS.index(kind))
        self.shape, self.kind = shape, kind
        self.xf = rng.uniform(-1, 1, (M, K)).astype(F) if kind == "f32" else None
        self.xq = rand8(rng, (M, K), U8 if kind == "u8" else S8)
        mk = lambda f_in, f_out: Params((rng.standard_normal((N, K)) * 0.02).astype(F), rng.standard_normal(N).astype(F),
                                        (1.0 / 127 if kind == "f32" else 0.031) * f_in, (0.5 if kind == "u8" else 1.0) * f_out)
        self.A, self.B = mk(1.0, 1.0), mk(IN_FACTOR, OUT_FACTOR)
        self.want = {"A": self.run(self.A), "B": self.run(self.B)}

    def operand(self, p):
        """the 8-bit operand the fc multiplies (f32 input: quantised with THE SET'S in_scale)"""
        return O.quant_flat_s8(self.xf, p.in_scale) if self.kind == "f32" else self.xq

    def run(self, p, wq=None, ws=None, bias="own", in_scale=None, out_scale=None, operand=None):
        return O.fc_i8(self.operand(p) if operand is None else operand, p.wq if wq is None else wq, p.ws if ws is None else ws,
                       p.in_scale if in_scale is None else in_scale, p.bias if isinstance(bias, str) else bias,
                       p.out_scale if out_scale is None else out_scale)

    def stale_kinds(self):
        return ["weights", "bias", "in_scale"] + (["out_scale", "comp"] if self.kind == "u8" else [])

    def stale(self, kind):
        A, B = self.A, self.B
        if kind == "weights":
            return self.run(B, wq=A.wq)
        if kind == "bias":
            return self.run(B, bias=A.bias)
        if kind == "in_scale":
            return self.run(B, in_scale=A.in_scale, operand=self.operand(B))
        if kind == "out_scale":
            return self.run(B, out_scale=A.out_scale)
        assert kind == "comp"
        return self.run(B, bias=None)


def fc_case(shape, kind):
    if (shape, kind) not in _fc_cases:
        _fc_cases[(shape, kind)] = FcCase(shape, kind)
    return _fc_cases[(shape, kind)]


def fc_f32_case(shape):
    """FP32 fc: (x, [(w, b) A, (w, b) B])"""
    M, N, K = shape
    rng = np.random.default_rng(91000 + M + N + K)
    x = rng.standard_normal((M, K)).astype(F)
    return x, [((rng.standard_normal((N, K)) * np.sqrt(1.0 / K)).astype(F), rng.standard_normal(N).astype(F)) for _ in range(2)]


# ---- composites ------------------------------------------------------------------------------------------------------------------------------
class Node:
    def __init__(self, name, spec, src, res=None):
        self.name, self.spec, self.src, self.res = name, spec, src, res


class Composite:
    """members in launch order; src / res name an input tensor ("x", "res") or an earlier member; live: the members the launch reads LIVE
    (every other member is COPIED when the composite is created)"""

    def __init__(self, name, nodes, inputs, live=()):
        self.name, self.nodes, self.inputs, self.live = name, nodes, inputs, frozenset(live)
        self.names = [n.name for n in nodes]
        self.written = [m for m in self.names if not m.startswith(("c3", "hc3"))]      # a chain's 3x3 edge stays in LDS
        self.A, self.B = {}, {}
        self._memo = {}

    def params(self, m, which):
        return (self.A if which == "A" else self.B)[m]

    def eval(self, pick):
        """{member: its output tensor} under pick = {member: "A" | "B"}; memoised per member on the choices it depends on"""
        out, key = dict(self.inputs), {k: (k,) for k in self.inputs}
        for n in self.nodes:
            key[n.name] = (n.name, pick[n.name], key[n.src], key.get(n.res))
            if key[n.name] not in self._memo:
                self._memo[key[n.name]] = run(n.spec, out[n.src], self.params(n.name, pick[n.name]), out.get(n.res))
            out[n.name] = self._memo[key[n.name]]
        return {m: out[m] for m in self.names}

    def all(self, which):
        return {m: which for m in self.names}

    def documented(self, updated):
        """after set_weights(B) on the members in `updated`: a copied member keeps A, a live one follows"""
        return {m: ("B" if m in updated and m in self.live else "A") for m in self.names}

    def updates(self):
        """the update steps the device test runs: each member alone, then all of them"""
        return [frozenset([m]) for m in self.names] + [frozenset(self.names)]

    def other_picks(self, doc):
        """every other old / new combination (<= 3 members), else every single flip of `doc` and its complement"""
        import itertools
        if len(self.names) <= 3:
            picks = [dict(zip(self.names, c)) for c in itertools.product("AB", repeat=len(self.names))]
        else:
            flip = lambda p, m: dict(p, **{m: "A" if p[m] == "B" else "B"})
            picks = [flip(doc, m) for m in self.names] + [{m: ("A" if doc[m] == "B" else "B") for m in self.names}]
        return [p for p in picks if p != doc]


def _fill(comp, rng, scales, bias=None):
    """draw A and B for every member: scales = {member: (in_scale, out_scale)}"""
    for n in comp.nodes:
        comp.A[n.name], comp.B[n.name] = draw_pair(rng, n.spec, *scales[n.name], bias=True if bias is None else bias[n.name])
    return comp


def _elt(geo, idt, mult=(1.0, 1.0), scale_res=S_RES, res_relu=True, **kw):
    return Spec(geo, idt, S8, 0, "elt", coeff=coeff_pair(mult), scale_res=scale_res, res_relu=res_relu, **kw)


# the shapes, restated from the device tests' own tables (tests/test_gpu_live_weights.py asserts them against those tables)
PAIR_CASE = (2, 14, 14, 64, 256, 64, 1, 0, 1)                 # test_gpu_parity.PAIR_CASES[0]
CHAIN_CASE = (64, 1, 9, S8, S8, 0, 0, 4)                      # the smallest of test_gpu_parity.CHAIN_CASES
CHAIN3_CASE = (64, 1, 7, 9, S8, S8, S8, 0, 0, 4)              # the smallest of test_gpu_parity.CHAIN3_CASES
HEAD_CASE = (256, 1, 9, 7, U8, S8, 1, None)                   # the smallest of test_gpu_parity.STRIDED_HEAD_CASES
STAGE_SHAPES = [(256, 2, 7, 9), (64, 2, 7, 9)]                # of P.STAGE_PROBE_SHAPES
TAIL_CASE = (2, 7, 9, 2, S8, 0)                               # test_gpu_stage_tail.TAIL_CASES[0]
STEM_IMAGE = (18, 23)
_composites = {}


def _blocks(C, N, H, W, nblk, first_dt=U8):
    """nblk [3x3 -> 1x1 + eltwise(relu) -> 1x1] blocks, block i + 1 reading block i's two outputs (tests/test_gpu_parity.py: _res4_blocks)"""
    nodes, scales, x, res, idt = [], {}, "x", "res", first_dt
    for k in range(nblk):
        odt2 = U8 if k % 2 == 0 else S8
        c3, a, b = "c3_%d" % k, "a_%d" % k, "b_%d" % k
        nodes += [Node(c3, Spec((N, H, W, C, C, 3, 1, 1), idt, U8, 1), x),
                  Node(a, _elt((N, H, W, C, 4 * C, 1, 0, 1), U8, scale_res=S_RES + 0.002 * k), c3, res),
                  Node(b, Spec((N, H, W, 4 * C, C, 1, 0, 1), S8, odt2, odt2 == U8), a)]
        scales.update({c3: (0.012 + 0.001 * k, 0.02), a: (0.02, 0.05), b: (S_SUM, 0.031)})
        x, res, idt = b, a, odt2
    return nodes, scales, idt


def _head(C, N, H, W, idt, mdt, res_relu, src, res, mult=UNEQ):
    oh, ow = (H + 2 - 3) // 2 + 1, (W + 2 - 3) // 2 + 1
    nodes = [Node("hc3", Spec((N, H, W, C, C, 3, 1, 2), idt, mdt, mdt == U8), src),
             Node("ha", _elt((N, oh, ow, C, 4 * C, 1, 0, 1), mdt, mult, scale_res=0.06, res_relu=res_relu, res_stride=2, res_hw=(H, W)), "hc3", res)]
    return nodes, {"hc3": (0.012 if idt == U8 else 0.024, 0.02), "ha": (0.02, 0.05)}


def _build(name):
    rng = np.random.default_rng(int.from_bytes(name.encode(), "little") % (2 ** 31))
    if name == "pair":
        N, H, W, C, K1, K2, k, pad, stride = PAIR_CASE
        nodes = [Node("a", Spec((N, H, W, C, K1, k, pad, stride), U8, S8, 0), "x"), Node("b", Spec((N, H, W, C, K2, k, pad, stride), U8, U8, 1), "x")]
        return _fill(Composite(name, nodes, {"x": rand8(rng, (N, H, W, C), U8)}), rng, {"a": (0.007, 0.05), "b": (0.007, 0.031)})
    if name == "chain1x1":
        C, N, HW, idt, odt2, relu2, res_relu, _ = CHAIN_CASE
        nodes = [Node("a", _elt((N, HW, HW, C, 4 * C, 1, 0, 1), idt, UNEQ, res_relu=res_relu), "x", "res"),
                 Node("b", Spec((N, HW, HW, 4 * C, C, 1, 0, 1), S8, odt2, relu2), "a")]
        inputs = {"x": rand8(rng, (N, HW, HW, C), idt), "res": rand8(rng, (N, HW, HW, 4 * C), S8)}
        return _fill(Composite(name, nodes, inputs), rng, {"a": (0.02, 0.05), "b": (S_SUM, 0.031)})
    if name == "chain3x3":
        C, N, H, W, idt, mdt, odt2, relu2, res_relu, _ = CHAIN3_CASE
        nodes = [Node("c3", Spec((N, H, W, C, C, 3, 1, 1), idt, mdt, mdt == U8), "x"),
                 Node("a", _elt((N, H, W, C, 4 * C, 1, 0, 1), mdt, UNEQ, res_relu=res_relu), "c3", "res"),
                 Node("b", Spec((N, H, W, 4 * C, C, 1, 0, 1), S8, odt2, relu2), "a")]
        inputs = {"x": rand8(rng, (N, H, W, C), idt), "res": rand8(rng, (N, H, W, 4 * C), S8)}
        return _fill(Composite(name, nodes, inputs), rng, {"c3": (0.024, 0.04), "a": (0.04, 0.05), "b": (S_SUM, 0.031)})
    if name == "head":
        C, N, H, W, idt, mdt, res_relu, _ = HEAD_CASE
        nodes, scales = _head(C, N, H, W, idt, mdt, res_relu, "x", "res")
        inputs = {"x": rand8(rng, (N, H, W, C), idt), "res": rand8(rng, (N, H, W, 4 * C), S8)}
        return _fill(Composite(name, nodes, inputs), rng, scales)
    if name.startswith("stage/"):
        C, N, H, W = STAGE_SHAPES[int(name[6:])]
        nodes, scales, _ = _blocks(C, N, H, W, 2)
        inputs = {"x": rand8(rng, (N, H, W, C), U8), "res": rand8(rng, (N, H, W, 4 * C), S8)}
        return _fill(Composite(name, nodes, inputs), rng, scales)
    if name == "stage_tail":
        N, H, W, nblk, mdt, res_relu = TAIL_CASE
        nodes, scales, last_dt = _blocks(256, N, H, W, nblk)
        hn, hs = _head(256, N, H, W, last_dt, mdt, res_relu, nodes[-1].name, nodes[-2].name)
        scales.update(hs)
        inputs = {"x": rand8(rng, (N, H, W, 256), U8), "res": rand8(rng, (N, H, W, 1024), S8)}
        return _fill(Composite(name, nodes + hn, inputs), rng, scales)
    if name == "xcd_stage":          # tests/test_gpu_stage.py: res5 at batch 1 - res5a with its projection shortcut and two identity blocks on 7 x 7
        N, H, W = 1, 7, 7
        nodes, scales = [Node("short", Spec((N, H, W, 1024, 2048, 1, 0, 1), S8, S8, 0), "x")], {"short": (0.05, 0.07)}
        x, short, s_x, s_short = "x", "short", 0.05, 0.07
        for b in range(3):
            a, m, e = "a%d" % b, "m%d" % b, "e%d" % b
            s_e = 0.06 + 0.01 * b
            nodes += [Node(a, Spec((N, H, W, 1024 if b == 0 else 2048, 512, 1, 0, 1), S8, U8, 1), x),
                      Node(m, Spec((N, H, W, 512, 512, 3, 1, 1), U8, U8, 1), a),
                      Node(e, Spec((N, H, W, 512, 2048, 1, 0, 1), U8, S8, 0, "elt", coeff=coeff_pair(UNEQ if b == 1 else (1.0, 1.0), s_e),
                                   scale_res=s_short, res_relu=True), m, short)]
            scales.update({a: (s_x, 0.03), m: (0.03, 0.025), e: (0.025, s_e)})
            x, short, s_x, s_short = e, e, s_e, s_e
        return _fill(Composite(name, nodes, {"x": rand8(rng, (N, H, W, 1024), S8)}), rng, scales)
    if name == "stem_pair":
        H, W = STEM_IMAGE
        ph, pw = _pool(np.zeros((1, (H + 6 - 7) // 2 + 1, (W + 6 - 7) // 2 + 1, 1), np.uint8)).shape[1:3]
        nodes = [Node("stem", Spec((1, H, W, 3, 64, 7, 3, 2), S8, U8, 1, pool=True), "x"),
                 Node("a", Spec((1, ph, pw, 64, 256, 1, 0, 1), U8, S8, 0), "stem"), Node("b", Spec((1, ph, pw, 64, 64, 1, 0, 1), U8, U8, 1), "stem")]
        comp = Composite(name, nodes, {"x": rand8(rng, (1, H, W, 3), S8)}, live=["stem"])
        return _fill(comp, rng, {"stem": (0.02, 0.1), "a": (0.01, 0.05), "b": (0.01, 0.031)})
    if name == "sep":
        from tests import sep_util as SU
        n, c, h, w, s, p, k = SU.GEOMETRIES[0]
        oh, ow = (h + 2 * p - 3) // s + 1, (w + 2 * p - 3) // s + 1
        nodes = [Node("dw", Spec((n, h, w, c, c, 3, p, s), U8, U8, 1, group=c), "x"), Node("pw", Spec((n, oh, ow, c, k, 1, 0, 1), U8, U8, 1), "dw")]
        return _fill(Composite(name, nodes, {"x": rand8(rng, (n, h, w, c), U8)}), rng, {"dw": (0.01, 0.03), "pw": (0.01, 0.05)})
    if name.startswith("ir/"):
        from tests import ir_util as IU
        cin, ce, cout, h, w, s, _, n = IU.GEOMETRIES[name[3:]]
        res = name[3:] == "i"          # "a" without the residual, "i" with it (x s8, Cin == Cout, stride 1): the fused eltwise reads the block's input
        oh, ow = (h + 2 - 3) // s + 1, (w + 2 - 3) // s + 1
        pr = _elt((n, oh, ow, ce, cout, 1, 0, 1), U8, UNEQ, scale_res=IU.IN_SCALE, res_relu=False) if res else Spec((n, oh, ow, ce, cout, 1, 0, 1), U8, S8, 0)
        nodes = [Node("expand", Spec((n, h, w, cin, ce, 1, 0, 1), S8, U8, 1), "x"), Node("dw", Spec((n, h, w, ce, ce, 3, 1, s), U8, U8, 1, group=ce), "expand"),
                 Node("project", pr, "dw", "x" if res else None)]
        return _fill(Composite(name, nodes, {"x": rand8(rng, (n, h, w, cin), S8)}), rng,
                     {"expand": (IU.IN_SCALE, 0.03), "dw": (0.01, 0.03), "project": (0.01, 0.05)})
    if name == "fire":
        from tests import fire_util as FU
        c, s, e1, e3, h, w, n = FU.GEOMETRIES["a"]
        nodes = [Node("squeeze", Spec((n, h, w, c, s, 1, 0, 1), U8, U8, 1), "x"), Node("e1", Spec((n, h, w, s, e1, 1, 0, 1), U8, U8, 1), "squeeze"),
                 Node("e3", Spec((n, h, w, s, e3, 3, 1, 1), U8, U8, 1), "squeeze")]
        return _fill(Composite(name, nodes, {"x": rand8(rng, (n, h, w, c), U8)}), rng, {"squeeze": (0.01, 0.03), "e1": (0.01, 0.04), "e3": (0.01, 0.05)})
    raise KeyError(name)


COMPOSITE_NAMES = ["pair", "chain1x1", "chain3x3", "head", "stage/0", "stage/1", "stage_tail", "xcd_stage", "stem_pair", "sep", "ir/a", "ir/i", "fire"]


def composite(name):
    if name not in _composites:
        _composites[name] = _build(name)
    return _composites[name]
