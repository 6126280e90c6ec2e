"""An op-list interpreter for the executor's legality tests: a list described in plain Python (tensors: name -> (NHWC shape, dtype); ops
in order), walked by the CPU oracle in LIST ORDER (`run_oracle`) and handed to the device executor (`build_net`). Unlike the model builders
it accepts what the C ABI accepts: a name written twice, in-place ops, readers anywhere. On top of it:

  * `PATTERNS`: the smallest list each rewrite of saber_hip_net_optimize accepts today, with calibrated scales (every edge between the rails);
  * perturbations: functions description -> description with exactly one change (an extra reader, a write before use, an in-place
    eltwise, a residual produced late, an op on lane 1, a rewritten source), and `diff` that says what changed;
  * `forced`: the description as if the rewrite had been applied ANYWAY - the pattern's ops as one step at the earliest position, its
    inner edges private to that step (never written: they read as POISON) - which is what the CPU test runs to show that every perturbed
    case tells a wrong rewrite from a right one;
  * `required`: the tensors somebody outside the pattern sees (an op that is no member of the producer's pattern, or nobody at all = an
    output). Those must have storage and be written in every selectable form.

Plain numpy + the CPU oracle; the device half imports the library lazily. TEST INFRASTRUCTURE ONLY."""
import numpy as np

from oracle import oracle as O
from tests import fire_util as FU

F32, S8, U8 = O.F32, O.S8, O.U8
NP_DT = {F32: np.float32, S8: np.int8, U8: np.uint8}
POISON = 77
FIRE, IR, SEP = 65536, 32768, 16384


# ---- descriptions ------------------------------------------------------------------------------------------------------------------------
class Desc:
    """tensors: {name: (shape, dtype)} in insertion order; ops: [dict] in list order, each with a unique "id" and the pattern instance it
    belongs to ("pat", None for an op a perturbation added); inputs: names the caller fills; scale: {name: float} of the 8-bit edges"""

    def __init__(self):
        self.tensors, self.ops, self.inputs, self.scale = {}, [], [], {}

    def copy(self):
        d = Desc()
        d.tensors, d.inputs, d.scale = dict(self.tensors), list(self.inputs), dict(self.scale)
        d.ops = [dict(o) for o in self.ops]      # (weights are shared: never modified)
        return d

    def index(self, op_id):
        return [o["id"] for o in self.ops].index(op_id)

    def op(self, op_id):
        return self.ops[self.index(op_id)]


def op_inputs(o):
    if o["kind"] == "fused":
        return [t for s in o["ops"] for t in op_inputs(s)]
    if o["kind"] == "elt":
        return [o["a"], o["b"]]
    if o["kind"] == "concat":
        return list(o["ins"])
    return [o["in"]]


def op_outputs(o):
    if o["kind"] == "fused":
        return [t for s in o["ops"] for t in op_outputs(s)]
    return [o["out"]]


_wq_cache = {}


def quantised(w):
    """(w_scale, wq) of a float weight array; cached by identity (weights are shared between descriptions and never modified)"""
    if id(w) not in _wq_cache:
        ws = O.weight_scales(w)
        _wq_cache[id(w)] = (w, ws, O.quant_weights(w, ws))
    return _wq_cache[id(w)][1:]


def _poison(shape, dt):
    return np.full(shape, np.nan, np.float32) if dt == F32 else np.full(shape, POISON, NP_DT[dt])


def _exec(o, desc, rd, wr):
    kd = o["kind"]
    if kd == "conv":
        x = rd(o, o["in"])
        ws, wq = quantised(o["w"])
        odt = desc.tensors[o["out"]][1]
        bp, sc = O.conv_i8_prepare(ws, o["b"], o["s_in"], o["s_out"], O.code_of(x), odt)
        wr(o["out"], O.conv_i8(x, wq, bp, sc, odt, int(o["relu"]), (o["pad"],) * 2, (o["stride"],) * 2, group=o["group"]))
    elif kd == "elt":
        a, b = rd(o, o["a"]), rd(o, o["b"])
        wr(o["out"], O.eltwise_i8(a, b, o["sa"], o["sb"], np.float32(o["c0"]), np.float32(o["c1"]), bool(o["relu"])))
    elif kd == "pool":
        x = rd(o, o["in"])
        if o.get("global"):
            wr(o["out"], O.pool_i8_nhwc(x, None, None, None, o["type"], global_pool=True))
        else:
            wr(o["out"], O.pool_i8_nhwc(x, (o["win"],) * 2, (o["stride"],) * 2, (o["pad"],) * 2, o["type"], floor_mode=o.get("floor", False)))
    elif kd == "concat":
        wr(o["out"], FU.concat_ref([rd(o, t) for t in o["ins"]], None))
    elif kd == "gpool_f32":      # the FP32 pooling op fed an 8-bit NHWC edge: dequantise on entry, then the global average
        wr(o["out"], O.pool_f32_nchw(O.dequant_nhwc_to_nchw(rd(o, o["in"]), o["scale"]), None, None, None, 1, global_pool=True))
    elif kd == "fc":             # f32 input: quantised on entry
        x = rd(o, o["in"])
        x = x.reshape(x.shape[0], -1)
        ws, wq = quantised(o["w"])
        wr(o["out"], O.fc_i8(O.quant_flat_s8(x, o["s_in"]), wq, ws, o["s_in"], o["b"]))
    elif kd == "softmax":
        wr(o["out"], O.softmax_f32(rd(o, o["in"])))
    else:
        raise ValueError(kd)


def run_oracle(desc, inputs):
    """Executes the ops in list order on a dict of numpy buffers; every non-input starts as POISON (NaN for f32). A name written twice or
    an in-place op simply overwrites. Returns (final contents of every buffer, {(op id, name): the value that op read} for the names
    written more than once)."""
    buf = {nm: _poison(sh, dt) for nm, (sh, dt) in desc.tensors.items()}
    for nm in desc.inputs:
        assert inputs[nm].shape == tuple(desc.tensors[nm][0]) and inputs[nm].dtype == NP_DT[desc.tensors[nm][1]], nm
        buf[nm] = inputs[nm].copy()
    writes = {nm: int(nm in desc.inputs) for nm in desc.tensors}
    for o in desc.ops:
        for t in op_outputs(o):
            writes[t] += 1
    seen = {}

    def rd(o, t):
        if writes[t] > 1:
            seen[(o["id"], t)] = buf[t].copy()
        return buf[t]

    def wr(t, v):
        assert v.dtype == NP_DT[desc.tensors[t][1]] and v.size == buf[t].size, (t, v.shape, buf[t].shape)
        buf[t] = v.reshape(buf[t].shape).copy()
    for o in desc.ops:
        if o["kind"] != "fused":
            _exec(o, desc, rd, wr)
            continue
        local = {}      # the step's private edges live here and nowhere else

        def rd_f(s, t):
            return local[t] if t in local else rd(s, t)

        def wr_f(t, v):
            if t in o["private"]:
                local[t] = v
            else:
                wr(t, v)
        for s in o["ops"]:
            _exec(s, desc, rd_f, wr_f)
    return buf, seen


def versions(desc):
    """[(name, writer index or -1 for an input, [reader indices])] of every value a tensor holds in the course of the list"""
    cur, out = {}, []
    for nm in desc.inputs:
        cur[nm] = (nm, -1, [])
        out.append(cur[nm])
    for i, o in enumerate(desc.ops):
        for t in op_inputs(o):
            if t in cur:
                cur[t][2].append(i)
        for t in op_outputs(o):
            cur[t] = (t, i, [])
            out.append(cur[t])
    return out


def written(desc):
    """names some op writes (their final contents are what a test compares)"""
    return [nm for nm in desc.tensors if any(nm in op_outputs(o) for o in desc.ops)]


def outputs(desc):
    """written names whose final value no op reads"""
    last = {}
    for v in versions(desc):
        last[v[0]] = v
    return [nm for nm in written(desc) if not last[nm][2]]


def unread(desc):
    """written names no op reads at all: what saber_hip_net_compact_arena keeps readable (a tensor an in-place op reads and writes is an
    inner edge to it)"""
    return [nm for nm in written(desc) if not any(nm in op_inputs(o) for o in desc.ops)]


def required(desc):
    """written names with a value somebody outside its producer's pattern sees: a reader that is no member of that pattern, or - for the
    final value - nobody at all. Those need storage and must be written whatever form is selected."""
    last, need, vs = {}, [], versions(desc)
    for v in vs:
        last[v[0]] = v
    for v in vs:
        nm, w, readers = v
        if w < 0:
            continue
        pat = desc.ops[w].get("pat")
        outside = any(pat is None or desc.ops[r].get("pat") != pat for r in readers)
        if outside or (last[nm] is v and not readers):
            if nm not in need:
                need.append(nm)
    return need


# ---- building patterns -------------------------------------------------------------------------------------------------------------------
class Builder:
    """Adds ops to a description while walking the oracle, so that every scale is the edge's own MAXABS scale (bytes between the rails)"""

    def __init__(self, seed):
        self.d, self.val, self.rng = Desc(), {}, np.random.default_rng(seed)

    def tensor(self, name, shape, dt, scale=None):
        assert name not in self.d.tensors, name
        self.d.tensors[name] = (tuple(shape), dt)
        if scale is not None:
            self.d.scale[name] = float(scale)

    def input(self, name, shape, dt, scale=0.02):
        self.tensor(name, shape, dt, scale)
        self.d.inputs.append(name)
        self.val[name] = self.rng.integers(0, 256, shape).astype(np.uint8) if dt == U8 else self.rng.integers(-128, 128, shape).astype(np.int8)
        return name

    def _run(self, o):
        def rd(_, t):
            return self.val[t]

        def wr(t, v):
            self.val[t] = v.reshape(self.d.tensors[t][0])
        _exec(o, self.d, rd, wr)

    def conv(self, op_id, pat, x, y, k, ksize=1, pad=0, stride=1, group=1, relu=False, odt=S8, bias=True, wstd=None):
        n, h, w, c = self.d.tensors[x][0]
        cg = c // group
        wstd = np.sqrt(2.0 / (cg * ksize * ksize)) if wstd is None else wstd
        wt = (self.rng.standard_normal((k, cg, ksize, ksize)) * wstd).astype(np.float32)
        b = (self.rng.standard_normal(k) * 0.5).astype(np.float32) if bias else None
        oh, ow = O.conv_out_hw(h, w, ksize, ksize, (pad, pad), (stride, stride), (1, 1))
        ws, wq = quantised(wt)
        bp, sc = O.conv_i8_prepare(ws, b, self.d.scale[x], 1.0, self.d.tensors[x][1], F32)
        f = O.conv_i8(self.val[x], wq, bp, sc, F32, int(relu), (pad, pad), (stride, stride), group=group)
        s_out = max(float(np.abs(f).max()), 1e-6) / 127.0
        self.tensor(y, (n, oh, ow, k), odt, s_out)
        o = {"kind": "conv", "id": op_id, "pat": pat, "lane": 0, "in": x, "out": y, "w": wt, "b": b, "s_in": self.d.scale[x], "s_out": s_out,
             "relu": bool(relu), "pad": pad, "stride": stride, "group": group}
        self.d.ops.append(o)
        self._run(o)
        return y

    def elt(self, op_id, pat, a, b, y, relu=False, m=(1.0, 1.0)):
        sa, sb = self.d.scale[a], self.d.scale[b]
        f = m[0] * self.val[a].astype(np.float64) * sa + m[1] * self.val[b].astype(np.float64) * sb
        s = max(float(np.abs(np.maximum(f, 0) if relu else f).max()), 1e-6) / 127.0
        c = 1.0 / s
        self.tensor(y, self.d.tensors[a][0], S8, s)
        o = {"kind": "elt", "id": op_id, "pat": pat, "lane": 0, "a": a, "b": b, "out": y, "sa": sa, "sb": sb,
             "c0": float(np.float32(m[0] * c)), "c1": float(np.float32(m[1] * c)), "relu": bool(relu)}
        self.d.ops.append(o)
        self._run(o)
        return y

    def pool(self, op_id, pat, x, y, win, stride, pad=0, ptype=0, floor=False, glob=False):
        n, h, w, c = self.d.tensors[x][0]
        oh, ow = (1, 1) if glob else O.pool_out_hw(h, w, (pad, pad), (win, win), (stride, stride), floor)
        self.tensor(y, (n, oh, ow, c), self.d.tensors[x][1], self.d.scale[x])
        o = {"kind": "pool", "id": op_id, "pat": pat, "lane": 0, "in": x, "out": y, "win": win, "stride": stride, "pad": pad, "type": ptype,
             "floor": floor, "global": glob}
        self.d.ops.append(o)
        self._run(o)
        return y

    def concat(self, op_id, pat, ins, y):
        sh = self.d.tensors[ins[0]][0]
        self.tensor(y, sh[:-1] + (sum(self.d.tensors[t][0][-1] for t in ins),), self.d.tensors[ins[0]][1], max(self.d.scale.get(t, 1.0) for t in ins))
        o = {"kind": "concat", "id": op_id, "pat": pat, "lane": 0, "ins": list(ins), "out": y}
        self.d.ops.append(o)
        self._run(o)
        return y

    def gpool_f32(self, op_id, pat, x, y):
        n, h, w, c = self.d.tensors[x][0]
        self.tensor(y, (n, c, 1, 1), F32)
        o = {"kind": "gpool_f32", "id": op_id, "pat": pat, "lane": 0, "in": x, "out": y, "scale": self.d.scale[x]}
        self.d.ops.append(o)
        self._run(o)
        return y

    def fc(self, op_id, pat, x, y, n_out):
        m = self.d.tensors[x][0][0]
        k = int(np.prod(self.d.tensors[x][0][1:]))
        wt = (self.rng.standard_normal((n_out, k)) * 0.05).astype(np.float32)
        b = self.rng.standard_normal(n_out).astype(np.float32)
        s_in = max(float(np.abs(self.val[x]).max()), 1e-6) / 127.0
        self.tensor(y, (m, n_out), F32)
        o = {"kind": "fc", "id": op_id, "pat": pat, "lane": 0, "in": x, "out": y, "w": wt, "b": b, "s_in": s_in}
        self.d.ops.append(o)
        self._run(o)
        return y

    def softmax(self, op_id, pat, x, y):
        self.tensor(y, self.d.tensors[x][0], F32)
        o = {"kind": "softmax", "id": op_id, "pat": pat, "lane": 0, "in": x, "out": y}
        self.d.ops.append(o)
        self._run(o)
        return y


class Pattern:
    """One instance of a rewrite's pattern inside a Builder's description.
    ops: its members' ids in list order;  inner: edges the rewrite (or a later site flag) may stop writing - the extra readers' targets;
    moved: (tensor, first id, last id) - the rewrite writes `tensor` at `first` instead of `last`;  source: (tensor, first id, last id) - the
    rewrite reads `tensor` at `last` instead of `first`;  elt: the id of its eltwise;  late: the tensor (an input of the list) that the
    "residual produced late" perturbation produces between the conv and the eltwise;  conv: the conv in front of the eltwise;
    lane: the op the lane perturbation moves;  out: its output;  flags: the optimize calls, in workloads.build_int8_net's order"""

    def __init__(self, name, tag, flags, ops, inner, out, moved=None, source=None, elt=None, conv=None, late=None, lane=None, at=None):
        self.name, self.tag, self.flags, self.ops, self.inner, self.out = name, tag, list(flags), list(ops), list(inner), out
        self.moved, self.source, self.elt, self.conv, self.late, self.lane = moved, source, elt, conv, late, lane or ops[0]
        self.at = at or ops[0]      # the op at whose position the rewritten pattern runs


FLAG_ORDER = [15, FIRE, IR, SEP, 64, 128, 512, 16 | 32 | 256 | 1024, 4096]      # workloads.build_int8_net (15 = 1 | 2 | 4 | 8)


def flags_for(patterns):
    """the optimize calls the patterns ask for, each once, in workloads.build_int8_net's order"""
    bits = 0
    for p in patterns:
        for f in p.flags:
            bits |= f
    return [f if f == 15 else f & bits for f in FLAG_ORDER if f & bits]


def _src(b, tag, src, shape, dt):
    return src if src is not None else b.input(tag + "x", shape, dt)


def pat_f1(b, tag="", src=None):
    """flag 1: 1x1 conv 64 -> 64 (-> s8) + eltwise with an external residual"""
    x = _src(b, tag, src, (1, 6, 7, 64), U8)
    if b.d.tensors[x][0][-1] % 64:
        return None
    t = b.conv(tag + "conv", tag, x, tag + "t", 64)
    r = b.input(tag + "r", b.d.tensors[t][0], S8, 0.05)
    e = b.elt(tag + "elt", tag, t, r, tag + "e", relu=True, m=(1.0, 0.5))
    return Pattern("f1", tag, [15], [tag + "conv", tag + "elt"], [t], e, moved=(e, tag + "conv", tag + "elt"), elt=tag + "elt", conv=tag + "conv",
                   late=r, lane=tag + "elt")


def pat_f4(b, tag="", src=None):
    """flag 4: the 7x7 / 2 stem conv + 3x3 / 2 max pooling (the only INT8 conv + pooling kernel)"""
    if src is not None:
        return None
    x = b.input(tag + "x", (1, 30, 30, 3), U8, 1 / 127.0)
    t = b.conv(tag + "conv", tag, x, tag + "t", 64, 7, 3, 2, relu=True, odt=U8, wstd=0.1)
    u = b.pool(tag + "pool", tag, t, tag + "u", 3, 2)
    return Pattern("f4", tag, [15], [tag + "conv", tag + "pool"], [t], u, moved=(u, tag + "conv", tag + "pool"), lane=tag + "pool")


def pat_f512(b, tag="", src=None):
    """flag 512: the fused stem conv + pooling and the sibling pair (256 + 64 channels) that alone reads the pooled tensor"""
    p = pat_f4(b, tag, src)
    if p is None:
        return None
    ya = b.conv(tag + "pa", tag, p.out, tag + "ya", 256)
    b.conv(tag + "pb", tag, p.out, tag + "yb", 64, relu=True, odt=U8)
    return Pattern("f512", tag, [15, 512], p.ops + [tag + "pa", tag + "pb"], p.inner + [p.out], ya, moved=(tag + "yb", tag + "pa", tag + "pb"),
                   source=(p.out, tag + "pa", tag + "pb"), lane=tag + "pb")


def pat_f128(b, tag="", src=None):
    """flag 128: 1x1 conv 1024 -> 64 on 5 x 3 pixels (an image-resident shape) + the INT8 global average pooling of its output"""
    x = _src(b, tag, src, (1, 5, 3, 1024), U8)
    n, h, w, c = b.d.tensors[x][0]
    if c != 1024 or h * w > 64:
        return None
    t = b.conv(tag + "conv", tag, x, tag + "t", 64)
    g = b.pool(tag + "gpool", tag, t, tag + "g", h, h, ptype=1, glob=True)
    return Pattern("f128", tag, [128], [tag + "conv", tag + "gpool"], [t], g, moved=(g, tag + "conv", tag + "gpool"), lane=tag + "gpool")


def pat_f2(b, tag="", src=None):
    """flag 2: two 1x1 / stride-2 convs 128 -> 128 and 128 -> 48 over one tensor (odd spatial dims, K2 no tile multiple)"""
    x = _src(b, tag, src, (1, 9, 7, 128), U8)
    if b.d.tensors[x][0][-1] % 64:
        return None
    ya = b.conv(tag + "ca", tag, x, tag + "ya", 128, stride=2)
    b.conv(tag + "cb", tag, x, tag + "yb", 48, stride=2, relu=True, odt=U8)
    return Pattern("f2", tag, [15], [tag + "ca", tag + "cb"], [], ya, moved=(tag + "yb", tag + "ca", tag + "cb"), source=(x, tag + "ca", tag + "cb"),
                   lane=tag + "cb")


def pat_f64(b, tag="", src=None):
    """flags 1 + 64: a shortcut's 1x1 / stride-2 max pooling (29 x 29 -> 15 x 15, 128 channels) read by the eltwise behind a 1x1 conv 64 -> 128"""
    if src is not None:
        return None
    sc = b.input(tag + "sc", (2, 29, 29, 128), S8, 0.043)
    x = b.input(tag + "x", (2, 15, 15, 64), U8)
    q = b.pool(tag + "pool", tag, sc, tag + "q", 1, 2, floor=True)
    t = b.conv(tag + "conv", tag, x, tag + "t", 128)
    e = b.elt(tag + "elt", tag, t, q, tag + "e", relu=True, m=(1.0, 0.5))
    return Pattern("f64", tag, [15, 64], [tag + "pool", tag + "conv", tag + "elt"], [q, t], e, source=(sc, tag + "pool", tag + "conv"),
                   moved=(e, tag + "conv", tag + "elt"), elt=tag + "elt", conv=tag + "conv", lane=tag + "pool", at=tag + "conv")


def pat_tail(b, tag="", src=None):
    """flags 8 + 4096: global average pooling (f32 out) of an s8 edge, the INT8 fc (512 -> 37) that quantises on entry, softmax"""
    x = _src(b, tag, src, (1, 3, 3, 512), S8)
    if b.d.tensors[x][0][-1] != 512 or b.d.tensors[x][1] != S8:
        return None
    g = b.gpool_f32(tag + "gpool", tag, x, tag + "g")
    y = b.fc(tag + "fc", tag, g, tag + "y", 37)
    p = b.softmax(tag + "softmax", tag, y, tag + "prob")
    return Pattern("tail", tag, [15, 4096], [tag + "gpool", tag + "fc", tag + "softmax"], [g, y], p, lane=tag + "softmax")


def pat_sep(b, tag="", src=None):
    """flag 16384: depthwise 3x3 (32 channels, 9 x 7, two images) + 1x1 conv 32 -> 64"""
    x = _src(b, tag, src, (2, 9, 7, 32), U8)
    c = b.d.tensors[x][0][-1]
    if c % 32:
        return None
    m = b.conv(tag + "dw", tag, x, tag + "m", c, 3, 1, 1, group=c, relu=True, odt=U8, wstd=0.4)
    y = b.conv(tag + "pw", tag, m, tag + "y", 64, relu=True, odt=U8)
    return Pattern("sep", tag, [SEP], [tag + "dw", tag + "pw"], [m], y, lane=tag + "pw")


def pat_ir(b, tag="", src=None):
    """flags 1 + 32768: 1x1 expand 16 -> 96, depthwise 3x3, 1x1 project 96 -> 16 (-> s8) + eltwise with the block's input (5 x 7, two images)"""
    x = _src(b, tag, src, (2, 5, 7, 16), S8)
    c = b.d.tensors[x][0][-1]
    if c != 16 or b.d.tensors[x][1] != S8:
        return None
    e = b.conv(tag + "ex", tag, x, tag + "e", 96, relu=True, odt=U8)
    d = b.conv(tag + "dw", tag, e, tag + "d", 96, 3, 1, 1, group=96, relu=True, odt=U8, wstd=0.4)
    p = b.conv(tag + "pj", tag, d, tag + "p", 16)
    y = b.elt(tag + "elt", tag, p, x, tag + "y", relu=False)
    return Pattern("ir", tag, [15, IR], [tag + "ex", tag + "dw", tag + "pj", tag + "elt"], [e, d, p], y, moved=(y, tag + "pj", tag + "elt"),
                   elt=tag + "elt", conv=tag + "pj", lane=tag + "dw")


def pat_irsep(b, tag="", src=None):
    """the same block without the residual: matches 32768 and - its last two ops - 16384 at once (the ordering cases)"""
    x = _src(b, tag, src, (2, 5, 7, 32), S8)
    if b.d.tensors[x][0][-1] != 32:
        return None
    e = b.conv(tag + "ex", tag, x, tag + "e", 96, relu=True, odt=U8)
    d = b.conv(tag + "dw", tag, e, tag + "d", 96, 3, 1, 1, group=96, relu=True, odt=U8, wstd=0.4)
    p = b.conv(tag + "pj", tag, d, tag + "p", 32)      # (K % 32 == 0: the separable kernel takes the last two ops)
    return Pattern("irsep", tag, [15, IR, SEP], [tag + "ex", tag + "dw", tag + "pj"], [e, d], p, lane=tag + "dw")


def pat_fire(b, tag="", src=None):
    """flag 65536: 1x1 squeeze 16 -> 16, 1x1 and 3x3 expand 16 -> 16 each, the u8 concat of the two (5 x 7, two images)"""
    x = _src(b, tag, src, (2, 5, 7, 16), U8)
    if b.d.tensors[x][0][-1] % 16:
        return None
    s = b.conv(tag + "sq", tag, x, tag + "s", 16, relu=True, odt=U8)
    a = b.conv(tag + "e1", tag, s, tag + "a", 16, relu=True, odt=U8)
    c = b.conv(tag + "e3", tag, s, tag + "b", 16, 3, 1, relu=True, odt=U8)
    # (the reference's concat takes the larger scale; the two are made equal here, as workloads.calibrate does, so that it is a copy)
    sc = max(b.d.scale[a], b.d.scale[c])
    for t, op_id in ((a, tag + "e1"), (c, tag + "e3")):
        b.d.scale[t] = sc
        b.d.op(op_id)["s_out"] = sc
        b._run(b.d.op(op_id))
    y = b.concat(tag + "cat", tag, [a, c], tag + "y")
    return Pattern("fire", tag, [FIRE], [tag + "sq", tag + "e1", tag + "e3", tag + "cat"], [s, a, c], y, lane=tag + "e3")


def pat_chain(b, tag="", src=None, blocks=2, c=64):
    """flags 1 + 16 + 32 (+ 256): `blocks` ResNet blocks [conv3x3 C -> C, conv1x1 C -> 4C + eltwise, conv1x1 4C -> C] at C = 64 on 7 x 9, two
    images, each reading the block before it (tests/block_table.py's shape and per-block table)"""
    from tests import block_table as BT
    if src is not None:
        return None
    x = b.input(tag + "x", (2, 7, 9, c), U8, 0.023)
    res = b.input(tag + "res", (2, 7, 9, 4 * c), S8, 0.043)
    ops, inner = [], []
    for k, (hand, relu1, res_relu, m) in enumerate(BT.TABLE[:blocks]):
        t0 = b.conv("%sb%d_3x3" % (tag, k), tag, x, "%st0_%d" % (tag, k), c, 3, 1, relu=True, odt=U8)
        t1 = b.conv("%sb%d_a" % (tag, k), tag, t0, "%st1_%d" % (tag, k), 4 * c, relu=bool(relu1))
        y1 = b.elt("%sb%d_elt" % (tag, k), tag, t1, res, "%sy1_%d" % (tag, k), relu=bool(res_relu), m=m)
        y2 = b.conv("%sb%d_b" % (tag, k), tag, y1, "%sy2_%d" % (tag, k), c, relu=hand == U8, odt=hand)
        ops += ["%sb%d_3x3" % (tag, k), "%sb%d_a" % (tag, k), "%sb%d_elt" % (tag, k), "%sb%d_b" % (tag, k)]
        inner += [t0, t1] + ([y1, y2] if k + 1 < blocks else [])
        x, res = y2, y1
    return Pattern("chain", tag, [15, 16 | 32], ops, inner, x, moved=(tag + "y1_0", tag + "b0_a", tag + "b0_elt"), elt=tag + "b0_elt", conv=tag + "b0_a",
                   lane=tag + "b0_3x3")


def pat_head(b, tag="", src=None):
    """flags 1 + 2 + 64 + 32 + 1024, the second loop of flag 32: a strided head - conv3x3 / 2 (C = 64), conv1x1 64 -> 256 + eltwise with the
    sub-sampled shortcut - that heads no chain, and the sibling pair (128 + 512 channels) that alone reads the sum (30 x 22 -> 15 x 11, two
    images: the smallest head + pair case of test_gpu_parity.HEAD_PAIR_CASES)"""
    if src is not None:
        return None
    sc = b.input(tag + "sc", (2, 30, 22, 256), S8, 0.043)
    x = b.input(tag + "x", (2, 30, 22, 64), S8, 0.023)
    q = b.pool(tag + "pool", tag, sc, tag + "q", 1, 2, floor=True)
    t0 = b.conv(tag + "3x3", tag, x, tag + "t0", 64, 3, 1, 2)
    t1 = b.conv(tag + "a", tag, t0, tag + "t1", 256)
    y1 = b.elt(tag + "elt", tag, t1, q, tag + "y1", relu=False, m=(1.0, -0.5))
    za = b.conv(tag + "pa", tag, y1, tag + "za", 128)
    b.conv(tag + "pb", tag, y1, tag + "zb", 512, relu=True, odt=U8)
    return Pattern("head", tag, [15, 64, 16 | 32 | 1024], [tag + "pool", tag + "3x3", tag + "a", tag + "elt", tag + "pa", tag + "pb"], [q, t0, t1, y1], za,
                   moved=(y1, tag + "a", tag + "elt"), source=(sc, tag + "pool", tag + "a"), elt=tag + "elt", conv=tag + "a", lane=tag + "3x3", at=tag + "a")


def pat_stage(b, tag="", src=None):
    """flag 256 on top: the same two blocks as one persistent launch (C = 64: selected through its choice word only)"""
    p = pat_chain(b, tag, src, 2)
    if p is not None:
        p.name, p.flags = "stage", [15, 16 | 32 | 256]
    return p


def pat_irchain(b, tag="", src=None):
    """1x1 conv 64 -> 256 + eltwise, then the 1x1 conv 256 -> 64 that reads the sum, behind a 1x1 conv and a depthwise conv: the last two
    match the chain flag 16, the first three the block flag 32768 where it takes the shape - the list both orders of the two flags see"""
    x = _src(b, tag, src, (2, 7, 9, 64), S8)
    if b.d.tensors[x][0][-1] != 64 or b.d.tensors[x][1] != S8:
        return None
    e = b.conv(tag + "ex", tag, x, tag + "e", 64, relu=True, odt=U8)
    d = b.conv(tag + "dw", tag, e, tag + "d", 64, 3, 1, 1, group=64, relu=True, odt=U8, wstd=0.4)
    p = b.conv(tag + "pj", tag, d, tag + "p", 64)
    y = b.elt(tag + "elt", tag, p, x, tag + "y", relu=False)
    z = b.conv(tag + "nx", tag, y, tag + "z", 64, relu=True, odt=U8)
    return Pattern("irchain", tag, [15, IR, 16 | 32], [tag + "ex", tag + "dw", tag + "pj", tag + "elt", tag + "nx"], [e, d, p, y], z, lane=tag + "dw")


PATTERNS = {"f1": pat_f1, "f4": pat_f4, "f128": pat_f128, "f2": pat_f2, "f64": pat_f64, "tail": pat_tail, "sep": pat_sep, "ir": pat_ir,
            "fire": pat_fire, "chain": pat_chain, "f512": pat_f512, "stage": pat_stage, "head": pat_head}
_SEEDS = {nm: 9100 + 17 * i for i, nm in enumerate(sorted(list(PATTERNS) + ["irsep", "irchain"]))}
_pattern_cache = {}


def pattern(name):
    """(description, input values, Pattern) of one pattern on its own; cached, never modified (perturbations copy)"""
    if name not in _pattern_cache:
        fn = dict(PATTERNS, irsep=pat_irsep, irchain=pat_irchain)[name]
        b = Builder(_SEEDS[name])
        p = fn(b)
        _pattern_cache[name] = (b.d, {nm: b.val[nm] for nm in b.d.inputs}, p)
    return _pattern_cache[name]


# ---- perturbations: description -> a new description with exactly one change ------------------------------------------------------------
READER_KINDS = ["elt_a", "elt_b", "pool1x1", "concat_last", "conv1x1"]
_reader_w = {}


def _new_input(d, inputs, name, shape, dt, seed):
    rng = np.random.default_rng(seed)
    d.tensors[name] = (tuple(shape), dt)
    d.inputs.append(name)
    d.scale[name] = 0.03
    inputs[name] = rng.integers(0, 256, shape).astype(np.uint8) if dt == U8 else \
        (rng.integers(-128, 128, shape).astype(np.int8) if dt == S8 else rng.standard_normal(shape).astype(np.float32))


def _reader_op(d, inputs, kind, t, out, op_id, seed):
    """an op of `kind` that reads tensor t into the new tensor `out` (None: the kind does not take t's dtype)"""
    shape, dt = d.tensors[t]
    base = {"id": op_id, "pat": None, "lane": 0}
    if kind in ("elt_a", "elt_b"):
        if dt != S8:
            return None
        _new_input(d, inputs, out + "_p", shape, S8, seed)
        d.tensors[out] = (shape, S8)
        a, b = (t, out + "_p") if kind == "elt_a" else (out + "_p", t)
        # (c = 0.5 / scale on both sides: the sum of two full-range bytes stays inside the rails)
        sa, sb = d.scale.get(a, 0.03), d.scale.get(b, 0.03)
        return dict(base, kind="elt", a=a, b=b, out=out, sa=sa, sb=sb, c0=float(np.float32(0.45 / sa)), c1=float(np.float32(0.45 / sb)), relu=False)
    if kind == "pool1x1":
        if dt == F32 or len(shape) != 4:
            return None
        d.tensors[out] = (shape, dt)
        return dict(base, kind="pool", out=out, win=1, stride=1, pad=0, type=0, floor=False, **{"in": t, "global": False})
    if kind == "concat_last":
        _new_input(d, inputs, out + "_p", shape, dt, seed)
        d.tensors[out] = (shape[:-1] + (2 * shape[-1],), dt)
        return dict(base, kind="concat", ins=[out + "_p", t], out=out)
    if kind == "conv1x1":
        if dt == F32 or len(shape) != 4:
            return None
        c = shape[-1]
        if c not in _reader_w:
            rng = np.random.default_rng(600 + c)
            _reader_w[c] = (rng.standard_normal((16, c, 1, 1)) * np.sqrt(1.0 / c)).astype(np.float32)
        s_in = d.scale.get(t, 0.03)
        d.tensors[out] = (shape[:-1] + (16,), S8)
        # out scale: the output's standard deviation is about 74 * s_in (uniform bytes) -> +-3 sigma inside the rails
        return dict(base, kind="conv", out=out, w=_reader_w[c], b=None, s_in=s_in, s_out=2.0 * s_in * (1.0 if dt == S8 else 2.0), relu=False, pad=0, stride=1, group=1, **{"in": t})
    raise ValueError(kind)


def extra_reader(desc, inputs, t, kind, at, tag="xr"):
    """one more reader of tensor t, of `kind`, inserted at list position `at` (len(ops) = the very last op)"""
    d, inputs = desc.copy(), dict(inputs)
    o = _reader_op(d, inputs, kind, t, tag + "_out", tag, 7000 + at)
    if o is None:
        return None
    d.ops.insert(at, o)
    return d, inputs


def reader_positions(desc, pat, t):
    """{label: list position} for an extra reader of t: directly after its producer, between the pattern's ops (the last place where the
    list allows it), after the whole pattern, as the very last op. Positions that coincide are named once."""
    prod = max(i for i, o in enumerate(desc.ops) if t in op_outputs(o))
    last = max(desc.index(i) for i in pat.ops)
    pos = {"after_producer": prod + 1}
    if last > prod + 1:
        pos["between"] = last
    pos["after_pattern"] = last + 1
    if len(desc.ops) > last + 1:
        pos["last"] = len(desc.ops)
    out, seen = {}, set()
    for k, v in pos.items():
        if v not in seen:
            out[k] = v
            seen.add(v)
    return out


def _writer_op(d, inputs, t, op_id, seed):
    """an op that writes tensor t from new inputs: an eltwise for s8, a 1x1 pooling (a copy) for u8"""
    shape, dt = d.tensors[t]
    if dt == F32:
        return None
    if dt == S8:
        for s in ("_p", "_q"):
            _new_input(d, inputs, op_id + s, shape, S8, seed + len(s) + ord(s[1]))
        return {"kind": "elt", "id": op_id, "pat": None, "lane": 0, "a": op_id + "_p", "b": op_id + "_q", "out": t, "sa": 0.03, "sb": 0.03,
                "c0": float(np.float32(0.45 / 0.03)), "c1": float(np.float32(-0.45 / 0.03)), "relu": False}
    _new_input(d, inputs, op_id + "_p", shape, U8, seed)
    return {"kind": "pool", "id": op_id, "pat": None, "lane": 0, "in": op_id + "_p", "out": t, "win": 1, "stride": 1, "pad": 0, "type": 0,
            "floor": False, "global": False}


def rewrite_before_use(desc, inputs, pat):
    """an op in front of the pattern writes the tensor the pattern later overwrites (pat.moved), and a 1x1 pooling reads that EARLIER value
    inside the window - after the pattern's first op, before the one that overwrites it"""
    t, first, last = pat.moved
    d, inputs = desc.copy(), dict(inputs)
    w = _writer_op(d, inputs, t, "rw_w", 7100)
    r = _reader_op(d, inputs, "pool1x1", t, "rw_out", "rw_r", 7101)
    if w is None or r is None:
        return None
    d.ops.insert(d.index(last), r)
    d.ops.insert(d.index(first), w)
    return d, inputs


def rewrite_source(desc, inputs, pat):
    """an op between the pattern's first and last reader of its source (pat.source) rewrites that source: the last one sees the new value"""
    t, first, last = pat.source
    d, inputs = desc.copy(), dict(inputs)
    w = _writer_op(d, inputs, t, "rs_w", 7200)
    if w is None:
        return None
    d.ops.insert(d.index(last), w)
    return d, inputs


def in_place(desc, inputs, pat, side):
    """the pattern's eltwise writes its own operand a (side 0) or b (side 1)"""
    d = desc.copy()
    e = d.op(pat.elt)
    e["out"] = e["a" if side == 0 else "b"]
    return d, dict(inputs)


def residual_late(desc, inputs, pat):
    """the residual - an input of the list so far - is produced by a 1x1 pooling (a copy of a new input) between the conv and the eltwise"""
    if pat.late is None:
        return None
    d, inputs = desc.copy(), dict(inputs)
    r = pat.late
    shape, dt = d.tensors[r]
    d.inputs.remove(r)
    inputs["late_src"] = inputs.pop(r)
    d.tensors["late_src"] = (shape, dt)
    d.scale["late_src"] = d.scale[r]
    d.inputs.append("late_src")
    d.ops.insert(d.index(pat.elt), {"kind": "pool", "id": "late", "pat": None, "lane": 0, "in": "late_src", "out": r, "win": 1, "stride": 1, "pad": 0,
                                    "type": 0, "floor": False, "global": False})
    return d, inputs


def on_lane(desc, inputs, op_id):
    d = desc.copy()
    d.op(op_id)["lane"] = 1
    return d, dict(inputs)


def perturbations(name):
    """{case name: (description, inputs)} of every perturbation that applies to the named pattern"""
    desc, inputs, pat = pattern(name)
    out = {}
    for t in pat.inner:
        for label, at in reader_positions(desc, pat, t).items():
            for kind in READER_KINDS:      # (a kind that does not take the tensor's dtype is passed by: the s8 eltwise on a u8 or f32 edge)
                r = extra_reader(desc, inputs, t, kind, at)
                if r is not None:
                    out["reader:%s:%s:%s" % (t, kind, label)] = r
    if name == "stage":      # (the control and the extra readers only)
        return out
    if name in ("f1", "f128"):      # (flags 1, 4 and 128 want their conv on lane 0; flag 4's stem conv uses the workspace and cannot leave it)
        out["lane:%s" % pat.ops[0]] = on_lane(desc, inputs, pat.ops[0])
    if pat.moved:
        r = rewrite_before_use(desc, inputs, pat)
        if r is not None:
            out["rewrite_before_use:%s" % pat.moved[0]] = r
    if pat.source:
        r = rewrite_source(desc, inputs, pat)
        if r is not None:
            out["rewrite_source:%s" % pat.source[0]] = r
    if pat.elt:
        out["in_place:a"] = in_place(desc, inputs, pat, 0)
        out["in_place:b"] = in_place(desc, inputs, pat, 1)
        r = residual_late(desc, inputs, pat)
        if r is not None:
            out["residual_late"] = r
    out["lane:%s" % pat.lane] = on_lane(desc, inputs, pat.lane)
    return out


def diff(a, b):
    """what a perturbation changed: (ids of the ops added, ids removed, [(id, field)] changed, ids whose relative order changed)"""
    ia, ib = [o["id"] for o in a.ops], [o["id"] for o in b.ops]
    added, removed = [i for i in ib if i not in ia], [i for i in ia if i not in ib]
    changed = []
    for o in a.ops:
        if o["id"] in ib:
            p = b.op(o["id"])
            for k in sorted(set(o) | set(p)):
                va, vb = o.get(k), p.get(k)
                same = va is vb or (not isinstance(va, np.ndarray) and not isinstance(vb, np.ndarray) and va == vb)
                if not same:
                    changed.append((o["id"], k))
    common_a, common_b = [i for i in ia if i in ib], [i for i in ib if i in ia]
    return added, removed, changed, [i for i, j in zip(common_a, common_b) if i != j]


# ---- the description as if the rewrite had been applied anyway ---------------------------------------------------------------------------
def forced(desc, pat):
    """the pattern's ops as ONE step at the position where the rewrite runs them (pat.at: its first op, where a moved write then happens -
    or, for the folded shortcut pooling, the conv that reads the pooling's source in its place), its inner edges private to the step (a
    removed edge: never written, readers see POISON). The other ops keep their order around that position."""
    d = desc.copy()
    members = [d.op(i) for i in pat.ops]
    at = d.index(pat.at)
    step = {"kind": "fused", "id": pat.tag + "fused", "pat": pat.tag, "lane": 0, "ops": members, "private": set(pat.inner)}
    rest = [o for o in d.ops if o["id"] not in pat.ops]
    n_before = len([o for o in d.ops[:at] if o["id"] not in pat.ops])
    d.ops = rest[:n_before] + [step] + rest[n_before:]
    return d


def compared(desc):
    """the tensors a GPU test compares whatever is selected: required(desc)"""
    return required(desc)


def share_changed(desc, inputs, pat):
    """the largest share of bytes, over the compared tensors, by which the forced description's answer differs from the right one"""
    want, _ = run_oracle(desc, inputs)
    got, _ = run_oracle(forced(desc, pat), inputs)
    best, where = 0.0, None
    for nm in compared(desc):
        w, g = want[nm], got[nm]
        s = float(np.mean((w != g) | (np.isnan(g) if g.dtype == np.float32 else False)))
        if s > best:
            best, where = s, nm
    return best, where


# ---- the device half ---------------------------------------------------------------------------------------------------------------------
def build_net(desc, flags_sequence):
    """S.Net of the description: tensors, ops, lanes where an op asks for one, then one optimize call per entry of flags_sequence in that
    order. NOT finalized (structure checks come first). Returns (net, [each call's return value])."""
    from anakin_amd import lib as L
    from anakin_amd import saber as S
    net = S.Net()
    for nm, (shape, dt) in desc.tensors.items():
        net.add_tensor(nm, shape, dt)
    for i, o in enumerate(desc.ops):
        kd = o["kind"]
        if kd == "conv":
            n, h, w, c = desc.tensors[o["in"]][0]
            p = S.ConvParam(o["w"], o["b"], o["group"], (o["pad"],) * 2, (o["stride"],) * 2, (1, 1), o["relu"])
            conv = S.SaberConv2D(True).init((n, c, h, w), p, desc.tensors[o["in"]][1], desc.tensors[o["out"]][1], o["s_in"], o["s_out"],
                                            in_layout=L.NHWC, out_layout=L.NHWC)
            net.add_conv(conv, o["in"], o["out"])
        elif kd == "elt":
            net.add_eltwise_i8(int(np.prod(desc.tensors[o["out"]][0])), o["sa"], o["sb"], o["c0"], o["c1"], o["relu"], o["a"], o["b"], o["out"])
        elif kd == "pool":
            n, h, w, c = desc.tensors[o["in"]][0]
            oh, ow = desc.tensors[o["out"]][0][1:3]
            win, st = ((h, w), (h, w)) if o.get("global") else ((o["win"],) * 2, (o["stride"],) * 2)
            net.add_pool_i8(n, h, w, c, oh, ow, win, st, (o["pad"],) * 2, o["type"], desc.tensors[o["in"]][1], desc.tensors[o["out"]][1], o["in"], o["out"])
        elif kd == "concat":
            net.add_concat(o["ins"], o["out"])
        elif kd == "gpool_f32":
            n, h, w, c = desc.tensors[o["in"]][0]
            net.add_pool_f32_from_i8(n, h, w, c, 1, 1, (h, w), (h, w), (0, 0), 1, desc.tensors[o["in"]][1], o["scale"], o["in"], o["out"])
        elif kd == "fc":
            m = desc.tensors[o["in"]][0][0]
            k = int(np.prod(desc.tensors[o["in"]][0][1:]))
            fc = S.SaberFc(True).init(m, o["w"].shape[0], k, o["w"], o["b"], desc.tensors[o["in"]][1], o["s_in"])
            net.add_fc(fc, o["in"], o["out"])
        elif kd == "softmax":
            net.add_softmax(desc.tensors[o["in"]][0][0], desc.tensors[o["in"]][0][1], o["in"], o["out"])
        else:
            raise ValueError(kd)
        if o.get("lane"):
            net.set_lane(i, o["lane"])
    return net, [net.optimize(f) for f in flags_sequence]


def branchy_desc():
    """the list of test_gpu_fire._branchy_net: x -> three eltwise ops -> concat3 -> two more eltwise ops; (description, x, coefficients)"""
    n, h, w, c = 2, 13, 13, 48
    x = np.random.default_rng(11).integers(-128, 128, (n, h, w, c)).astype(np.int8)
    d = Desc()
    d.tensors["x"] = ((n, h, w, c), S8)
    d.inputs.append("x")
    coeffs = {"a": 0.5, "b": 0.25, "c": 0.75}
    elt = {"kind": "elt", "pat": None, "lane": 0, "sa": 1.0, "sb": 1.0}
    for nm in ("a", "b", "c"):
        d.tensors[nm] = ((n, h, w, c), S8)
        d.ops.append(dict(elt, id=nm, a="x", b="x", out=nm, c0=coeffs[nm], c1=coeffs[nm], relu=False))
    for nm in ("cat", "out", "out2"):
        d.tensors[nm] = ((n, h, w, 3 * c), S8)
    d.ops.append({"kind": "concat", "id": "cat", "pat": None, "lane": 0, "ins": ["a", "b", "c"], "out": "cat"})
    d.ops.append(dict(elt, id="out", a="cat", b="cat", out="out", c0=0.5, c1=0.5, relu=True))
    d.ops.append(dict(elt, id="out2", a="out", b="out", out="out2", c0=1.0, c1=0.5, relu=False))
    return d, x, coeffs
