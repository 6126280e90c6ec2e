"""saber_hip_conv2d_set_weights / saber_hip_fc_set_weights on LIVE ops (include/saber_hip.h: "every packing of the op follows the new weights
and bias ... and the kernel selection stays"; "pairs, chains and stages COPY their members' weights when they are created").

Single ops: run with parameter set A, set_weights(B), run, set_weights(A), run - in every kernel form the op accepts. After each step the
selection is unchanged and the output equals the oracle's for the set just given and a fresh op's built with it under the same set_tile code.
Composite launches: built from members holding A; then set_weights(B) on one member at a time and on all of them, and every form of the
composite is run: a COPIED member's change must not reach the output (bit for bit the earlier run), a LIVE member's must - never a mix.
tests/test_live_weights_cpu.py proves on the CPU that every case here tells the right answer from each stale or mixed one."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from anakin_amd import lib as L  # noqa: E402
from anakin_amd import saber as S  # noqa: E402
from oracle import oracle as O  # noqa: E402
from tests import int8_probe as P  # noqa: E402
from tests import live_weights_util as U  # noqa: E402
from tests.test_gpu_int8_probe import _forms  # noqa: E402  (the selection an op starts with + every code set_tile accepts, one per kernel name)
from tests.test_gpu_parity import FP32_RTOL  # noqa: E402

SENTINEL = 77
F32, S8, U8 = U.F32, U.S8, U.U8
TORCH_DT = {F32: torch.float32, S8: torch.int8, U8: torch.uint8}


@pytest.fixture(scope="module", autouse=True)
def _device():
    L.require_device()  # fail loudly: no fallback path exists


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def blank(want):
    """a device tensor of want's shape and dtype, every element the sentinel"""
    return torch.full(want.shape, SENTINEL, dtype=torch.from_numpy(want[:0]).dtype, device="cuda")


def same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        i = tuple(int(v) for v in bad[0])
        raise AssertionError("%s: %d of %d outputs differ, first at %s: got %s, want %s" % (what, len(bad), want.size, i, got[i], want[i]))


def _spelled(p, spelling):
    """(weights, w_scale) as f32 weights the library quantises, or as the s8 weights + w_scale the oracle quantised"""
    return (p.w, None) if spelling == "f32" else (p.wq, p.ws)


def make_op(spec, p, spelling="f32"):
    N, H, W, C, K, k, pad, stride = spec.geo
    w, ws = _spelled(p, spelling)
    cp = S.ConvParam(w, p.bias, spec.group, spec.pad, spec.stride, (1, 1), bool(spec.relu), ws)
    if spec.mode == "elt":
        cp.res_mode, cp.res_relu, cp.sum_scale, cp.coeff, cp.scale_res = L.RES_ELTWISE, spec.res_relu, 1.0, spec.coeff, spec.scale_res
        if spec.res_stride > 1:
            cp.res_stride, cp.res_hw = spec.res_stride, spec.res_hw
    elif spec.mode == "sum":
        cp.res_mode, cp.res_relu, cp.sum_scale, cp.res_dtype = L.RES_SUM_INPLACE, False, spec.sum_scale, spec.odt
    if spec.pool:
        op = S.SaberConv2DPooling().init((N, C, H, W), cp, L.POOL_MAX, (3, 3), (2, 2), (0, 0), spec.idt, spec.odt, p.in_scale, p.out_scale, in_layout=L.NHWC)
        assert op.fused
        return op
    return S.SaberConv2D(True).init((N, C, H, W), cp, spec.idt, spec.odt, p.in_scale, p.out_scale)


def set_w(op, p, spelling="f32"):
    w, ws = _spelled(p, spelling)
    (op.conv if isinstance(op, S.SaberConv2DPooling) else op).set_weights(w, p.bias, ws, p.in_scale, p.out_scale)


def tile_of(op):
    return L.load().saber_hip_conv2d_get_tile(op.h)


def run_op(op, c, which=None):
    """one launch of a single-op case on sentinel-filled (or, in-place sum, the case's previous) output bytes"""
    y = dev(c.prev) if c.prev is not None else blank(c.want["A"])
    op.dispatch(dev(c.x), y, dev(c.res)) if c.res is not None else op.dispatch(dev(c.x), y)
    return host(y)


# ---- single convolutions ----------------------------------------------------------------------------------------------------------------
def _a_b_a(c, forms_seen):
    """A, B, A on one op in every form; the fresh ops are built once per case and follow the live op's set_tile code"""
    live = make_op(c.spec, c.A)
    fresh = {"A": make_op(c.spec, c.A), "B": make_op(c.spec, c.B, "s8")}
    forms = [(None, live.algo())] if c.spec.pool else _forms(live)
    launches = 0
    for fi, (code, algo) in enumerate(forms):
        spell = ("f32", "s8") if fi % 2 == 0 else ("s8", "f32")          # f32 then s8 + w_scale, and the reverse
        outs = []
        for step, which in enumerate("ABA"):
            set_w(live, c.A if which == "A" else c.B, spell[step % 2])
            if code is not None:
                if step == 0:
                    live.set_tile(code)
                    selected = tile_of(live)
                fresh[which].set_tile(code)
                assert tile_of(live) == selected, (c.name, algo, which, hex(tile_of(live)), hex(selected))
            assert live.algo() == algo, (c.name, which, live.algo(), algo)
            got = run_op(live, c)
            same(got, c.want[which], "%s, %s, step %d (%s)" % (c.name, algo, step, which))
            same(got, run_op(fresh[which], c), "%s, %s, step %d (%s) against a fresh op" % (c.name, algo, step, which))
            outs.append(got)
            launches += 2
        assert not np.array_equal(outs[0], outs[1]), (c.name, algo)
        forms_seen.add(algo)
    return launches


FAMILY = {"pw_k64": "igemm_i8", "pw_k72": "igemm_i8", "pw_k34": "igemm_i8", "c3x3": "halo3x3_i8", "img3x3": "img3x3_i8", "imgres1x1": "imgres1x1_i8",
          "imgres3x3": "imgres3x3_i8", "stem": "stem7x7s2_i8", "stempool18x23": "maxpool"}
# the forms that have no in-place sum (tests/test_gpu_int8_probe.py: REFUSES)
NO_SUM = ("imgres1x1", "imgres3x3")


@pytest.mark.parametrize("name", U.case_names())
def test_conv_i8_follows_a_second_set_weights_in_every_form(name):
    seen = set()
    launches = _a_b_a(U.case(name), seen)
    print("%s: %d launches, %d kernel forms: %s" % (name, launches, len(seen), " ".join(sorted(seen))))
    g, epi, combo = name.split("/")
    if not (epi == "sum" and g in NO_SUM) and combo != "s8f32":          # the geometry reaches the kernel family it is here for (8-bit outputs)
        assert any(FAMILY[g] in a for a in seen), (name, sorted(seen))


@pytest.mark.parametrize("geometry", ["pw_k64", "c3x3", "imgres1x1", "stem"])
def test_conv_i8_bias_comes_and_goes(geometry):
    """bias -> None -> bias and None -> bias -> None: has_bias follows each call"""
    c = U.case("%s/plain/u8s8" % geometry)
    for first_none in (False, True):
        sets = [c.A.but(bias=None) if first_none else c.A, c.B if first_none else c.B.but(bias=None)]
        wants = [U.run(c.spec, c.x, p) for p in sets]
        assert U.share(wants[1], U.run(c.spec, c.x, c.B.but(bias=None) if first_none else c.B)) >= U.MIN_SHARE      # (with / without B's bias)
        live = make_op(c.spec, sets[0])
        for code, algo in _forms(live):
            for step in (0, 1, 0):
                set_w(live, sets[step])
                live.set_tile(code)
                same(run_op(live, c), wants[step], "%s, %s, first bias %s, set %d" % (c.name, algo, "None" if first_none else "given", step))


GPOOL_EPILOGUES = ["plain/u8u8", "plain/s8s8", "plain/u8s8", "elt/u8", "elt/s8"]


@pytest.mark.parametrize("geometry", ["imgres1x1", "imgres3x3"])
def test_conv_with_fused_global_pooling_follows_a_second_set_weights(geometry):
    """saber_hip_conv2d_set_global_pooling: the op then has the image-resident kernel alone, with a packing of its own - y and y_pool after
    A, B, A, against the oracle and a fresh op"""
    for epi in GPOOL_EPILOGUES:
        c = U.case("%s/%s" % (geometry, epi))
        pooled = {k: O.pool_i8_nhwc(v, None, None, None, 1, global_pool=True) for k, v in c.want.items()}
        assert U.share(pooled["A"], pooled["B"]) >= U.MIN_SHARE, (c.name, U.share(pooled["A"], pooled["B"]))

        def run(op):
            y, yp = blank(c.want["A"]), blank(pooled["A"])
            op.dispatch_gpool(dev(c.x), y, yp, None if c.res is None else dev(c.res))
            return host(y), host(yp)
        live = make_op(c.spec, c.A).set_global_pooling()
        algo, outs = live.algo(), []
        for step, which in enumerate("ABA"):
            set_w(live, c.A if which == "A" else c.B, ("f32", "s8")[step % 2])
            assert live.algo() == algo, (c.name, live.algo(), algo)
            y, yp = run(live)
            same(y, c.want[which], "%s + global pooling, y, step %d (%s)" % (c.name, step, which))
            same(yp, pooled[which], "%s + global pooling, y_pool, step %d (%s)" % (c.name, step, which))
            fy, fyp = run(make_op(c.spec, c.A if which == "A" else c.B).set_global_pooling())
            same(y, fy, "%s + global pooling, y against a fresh op" % c.name)
            same(yp, fyp, "%s + global pooling, y_pool against a fresh op" % c.name)
            outs.append(y)
        assert not np.array_equal(outs[0], outs[1]), c.name


# ---- fully connected ----------------------------------------------------------------------------------------------------------------------
FC_IGEMM_CODE = 0 | (1 << 8) | (1 << 16)          # the register-staged implicit GEMM (the small-batch kernel is the static choice at <= 16 rows)


@pytest.mark.parametrize("shape", U.FC_SHAPES)
@pytest.mark.parametrize("kind", U.FC_INPUTS)
def test_fc_i8_follows_a_second_set_weights(shape, kind):
    """INT8 fc, small-batch kernel and implicit GEMM: dispatch, dispatch_q (an s8 operand) and dispatch_softmax after A, B, A"""
    c = U.fc_case(shape, kind)
    M, N, K = shape
    idt = {"s8": L.S8, "u8": L.U8, "f32": L.F32}[kind]

    def make(p, spelling="f32"):
        w, ws = _spelled(p, spelling)
        return S.SaberFc(True).init(M, N, K, w, p.bias, idt, p.in_scale, p.out_scale, w_scale=ws)

    def run(fc, how, p):
        y, prob = torch.full((M, N), float(SENTINEL), device="cuda"), torch.full((M, N), float(SENTINEL), device="cuda")
        if how == "dispatch":
            fc.dispatch(dev(c.xf if kind == "f32" else c.xq), y)
        elif how == "dispatch_q":
            fc.dispatch_q(dev(c.operand(p)), y)
        else:
            fc.dispatch_softmax(dev(c.xf if kind == "f32" else c.xq), y, prob)
        return host(y), host(prob)
    live = make(c.A)
    assert live.algo().startswith("fc_i8_small"), live.algo()
    for form in (None, FC_IGEMM_CODE):
        fresh = {"A": make(c.A), "B": make(c.B, "s8")}
        if form is not None:
            for fc in [live] + list(fresh.values()):
                fc.set_tile(form)
            assert live.algo().startswith("igemm_i8"), live.algo()
        algo, outs = live.algo(), []
        for step, which in enumerate("ABA"):
            p = c.A if which == "A" else c.B
            w, ws = _spelled(p, ("f32", "s8")[step % 2])
            live.set_weights(w, p.bias, ws, p.in_scale, p.out_scale)
            assert live.algo() == algo, (shape, kind, live.algo(), algo)
            for how in ["dispatch"] + (["dispatch_q"] if kind != "u8" else []) + ["dispatch_softmax"]:
                y, prob = run(live, how, p)
                same(y, c.want[which], "fc %s %s, %s, %s, step %d (%s)" % (shape, kind, algo, how, step, which))
                same(y, run(fresh[which], how, p)[0], "fc %s %s, %s, %s, step %d against a fresh op" % (shape, kind, algo, how, step))
                if how == "dispatch_softmax":
                    sm = O.softmax_f32(c.want[which])
                    assert np.abs(prob - sm).max() <= FP32_RTOL * sm.max(), (shape, kind, algo, step, np.abs(prob - sm).max())
            outs.append(y)
        assert not np.array_equal(outs[0], outs[1]), (shape, kind, algo)
    # bias -> None -> bias, None -> bias -> None
    for first_none in (False, True):
        sets = [c.A.but(bias=None) if first_none else c.A, c.B if first_none else c.B.but(bias=None)]
        live = make(sets[0])
        for step in (0, 1, 0):
            p = sets[step]
            live.set_weights(p.w, p.bias, None, p.in_scale, p.out_scale)
            same(run(live, "dispatch", p)[0], c.run(p), "fc %s %s, first bias %s, set %d" % (shape, kind, "None" if first_none else "given", step))


@pytest.mark.parametrize("shape", U.FC_SHAPES)
@pytest.mark.parametrize("split_k", [False, True], ids=["default", "split_k"])
def test_fc_f32_follows_a_second_set_weights(shape, split_k):
    """FP32 fc, the default kernel and the split-K form (opt-in through the environment, read by set_weights): A, B, A and bias -> None -> bias,
    on test_fc_f32_split_k_and_softmax_in_one_launch's two FP32 criteria"""
    M, N, K = shape
    x, sets = U.fc_f32_case(shape)
    sets = [sets[0], sets[1], sets[0], (sets[1][0], None), sets[0]]
    if split_k:
        os.environ["SABER_HIP_FC_F32_SPLITK"] = "1"
    try:
        live = S.SaberFc(False).init(M, N, K, sets[0][0], sets[0][1], L.F32)
        assert live.algo() == ("fc_f32_splitk_16xk4" if split_k else "fc_f32_small_16xk4"), live.algo()
        algo, prev = live.algo(), None
        for step, (w, b) in enumerate(sets):
            live.set_weights(w, b)
            assert live.algo() == algo, (live.algo(), algo)
            want = O.fc_f32(x, w, b)
            y, prob = torch.full((M, N), float(SENTINEL), device="cuda"), torch.full((M, N), float(SENTINEL), device="cuda")
            live.dispatch(dev(x), y)
            got = host(y)
            a = np.abs(got - want).max() / np.abs(want).max()
            e = (np.abs(got - want) / (np.abs(want) + np.abs(want).mean())).max()
            print("fc f32 %s %s step %d: %.2e %.2e" % (shape, algo, step, a, e))
            assert a <= FP32_RTOL and e <= FP32_RTOL, (shape, algo, step, a, e)
            fresh = S.SaberFc(False).init(M, N, K, w, b, L.F32)
            assert fresh.algo() == algo
            yf = torch.empty_like(y)
            fresh.dispatch(dev(x), yf)
            same(got, host(yf), "fc f32 %s %s step %d against a fresh op" % (shape, algo, step))
            y.fill_(float(SENTINEL))
            live.dispatch_softmax(dev(x), y, prob)
            sm = O.softmax_f32(want)
            assert np.abs(host(prob) - sm).max() <= FP32_RTOL * sm.max() and np.abs(host(y) - want).max() <= FP32_RTOL * np.abs(want).max(), (shape, algo, step)
            assert prev is None or not np.array_equal(prev, got), (shape, algo, step)
            prev = got
    finally:
        os.environ.pop("SABER_HIP_FC_F32_SPLITK", None)


# ---- composite launches -------------------------------------------------------------------------------------------------------------------
def _codes(obj, hi):
    """every form code the composite's set_tile accepts"""
    keep, out = obj.tile(), []
    for code in range(1, hi + 1):
        try:
            obj.set_tile(code)
        except L.SaberHipError:
            continue
        out.append(code)
    obj.set_tile(keep)
    return out


def _outs(comp, names):
    w = comp.eval(comp.all("A"))
    return {m: blank(w[m]) for m in names}


def _host(outs):
    return {m: host(t) for m, t in outs.items()}


def drive(comp, ops, forms):
    """forms: [(label, fn)], fn() -> {member: output}. Every form under A; then set_weights(B) on each member alone and on all of them - the
    documented combination in every form, bit for bit the first run where every updated member is a copy - and A again."""
    first = {}
    want = comp.eval(comp.all("A"))
    for label, fn in forms:
        first[label] = fn()
        for m, got in first[label].items():
            same(got, want[m], "%s, %s, built from A: %s" % (comp.name, label, m))
    runs = len(forms)
    for updated in comp.updates():
        for i, m in enumerate(sorted(updated)):
            set_w(ops[m], comp.B[m], ("f32", "s8")[i % 2])
        doc = comp.documented(updated)
        want = comp.eval(doc)
        for label, fn in forms:
            for m, got in fn().items():
                same(got, want[m], "%s, %s, after set_weights(B) on %s: %s" % (comp.name, label, sorted(updated), m))
                if doc == comp.all("A"):
                    same(got, first[label][m], "%s, %s, after set_weights(B) on %s: %s against the first run" % (comp.name, label, sorted(updated), m))
            runs += 1
        for m in updated:
            set_w(ops[m], comp.A[m])
    for label, fn in forms:
        for m, got in fn().items():
            same(got, first[label][m], "%s, %s, after set_weights(A) again: %s" % (comp.name, label, m))
    print("%s: %d members (%s live), %d forms, %d launches" % (comp.name, len(comp.names), sorted(comp.live) or "none", len(forms), runs + len(forms)))


def _ops(comp):
    return {n.name: make_op(n.spec, comp.A[n.name]) for n in comp.nodes}


def test_sibling_pair_keeps_its_members_first_weights():
    import tests.test_gpu_parity as TP
    assert U.PAIR_CASE == TP.PAIR_CASES[0]
    comp = U.composite("pair")
    ops = _ops(comp)
    pair = S.SaberConvPair(ops["a"], ops["b"])
    x = dev(comp.inputs["x"])

    def form(code):
        def fn():
            pair.set_tile(code)
            o = _outs(comp, ["a", "b"])
            pair.dispatch(x, o["a"], o["b"])
            return _host(o)
        return fn
    drive(comp, ops, [(algo, form(code)) for code, algo in _forms(pair)])
    # set_weights on the pair op itself: refused, and the pair goes on computing what it did
    p = comp.B["a"]
    w = np.concatenate([comp.B["a"].w, comp.B["b"].w])
    rc = L.load().saber_hip_conv2d_set_weights(pair.h, w.ctypes.data, L.F32, None, None, p.in_scale, p.out_scale)
    assert rc == -2, rc          # SABER_HIP_INVALID_VALUE
    got = form(_forms(pair)[0][0])()
    want = comp.eval(comp.all("A"))
    same(got["a"], want["a"], "pair after the refused set_weights: a")
    same(got["b"], want["b"], "pair after the refused set_weights: b")


def _chain_forms(comp, chain, names, x, res):
    def form(code):
        def fn():
            chain.set_tile(code)
            o = _outs(comp, names)
            chain.dispatch(x, res, *[o[m] for m in names])
            assert chain.tile() == code, (chain.tile(), code)
            return _host(o)
        return fn
    codes = _codes(chain, 15)
    assert len(codes) >= 2, codes
    return [("code %d" % c, form(c)) for c in codes]


def test_conv1x1_chain_keeps_its_members_first_parameters():
    """the chain's first conv carries the fused eltwise with (1, -0.5) and out_scale_B != out_scale_A: a chain that read the member's current
    out_scale beside its own copy of the member's packing would compute neither A nor B"""
    import tests.test_gpu_parity as TP
    assert U.CHAIN_CASE == min(TP.CHAIN_CASES, key=lambda c: c[1] * c[2] * c[2] * c[0] * c[0])      # by multiply-adds
    comp = U.composite("chain1x1")
    ops = _ops(comp)
    chain = S.SaberConvChain(ops["a"], ops["b"])
    drive(comp, ops, _chain_forms(comp, chain, ["a", "b"], dev(comp.inputs["x"]), dev(comp.inputs["res"])))


def test_conv3x3_chain_keeps_its_members_first_parameters():
    import tests.test_gpu_parity as TP
    assert U.CHAIN3_CASE == min(TP.CHAIN3_CASES, key=lambda c: c[1] * c[2] * c[3] * c[0] * c[0])
    comp = U.composite("chain3x3")
    ops = _ops(comp)
    chain = S.SaberConvChain(ops["a"], ops["b"], conv3x3=ops["c3"])
    drive(comp, ops, _chain_forms(comp, chain, ["a", "b"], dev(comp.inputs["x"]), dev(comp.inputs["res"])))


def test_strided_head_keeps_its_members_first_parameters():
    import tests.test_gpu_parity as TP
    assert U.HEAD_CASE == min(TP.STRIDED_HEAD_CASES, key=lambda c: c[1] * c[2] * c[3] * c[0] * c[0])
    comp = U.composite("head")
    ops = _ops(comp)
    chain = S.SaberConvChain(ops["ha"], None, conv3x3=ops["hc3"])
    drive(comp, ops, _chain_forms(comp, chain, ["ha"], dev(comp.inputs["x"]), dev(comp.inputs["res"])))


def _stage_parts(comp, ops, nblk):
    chains = [S.SaberConvChain(ops["a_%d" % k], ops["b_%d" % k], conv3x3=ops["c3_%d" % k]) for k in range(nblk)]
    names = [m for k in range(nblk) for m in ("a_%d" % k, "b_%d" % k)]
    x, res = dev(comp.inputs["x"]), dev(comp.inputs["res"])

    def chain_form(code):
        def fn():
            o = _outs(comp, names)
            cx, cr = x, res
            for k, ch in enumerate(chains):
                ch.set_tile(code)
                ch.dispatch(cx, cr, o["a_%d" % k], o["b_%d" % k])
                cx, cr = o["b_%d" % k], o["a_%d" % k]
            return _host(o)
        return fn
    return chains, names, x, res, [("chains, code %d" % c, chain_form(c)) for c in _codes(chains[0], 15)]


def _stage_fn(comp, stage, names, nblk, x, res, tail=None):
    def fn():
        o = _outs(comp, names + ([tail] if tail else []))
        stage.dispatch(x, res, [o["a_%d" % k] for k in range(nblk)], [o["b_%d" % k] for k in range(nblk)], o[tail] if tail else None)
        return _host(o)
    return fn


@pytest.mark.parametrize("index", [0, 1])
def test_chain_stage_keeps_its_chains_first_parameters(index):
    """a stage launch of two block chains, and the chains themselves in every form they accept (at C = 256 the four-workgroup form is a
    one-block stage of its own): all of them the same bytes, whatever a member is given afterwards. And a stage built AFTER a member's second
    set_weights copies the chain's stored parameters, not the member's new ones: it equals the chain it was built from."""
    assert U.STAGE_SHAPES[index] in P.STAGE_PROBE_SHAPES
    comp = U.composite("stage/%d" % index)
    ops = _ops(comp)
    chains, names, x, res, forms = _stage_parts(comp, ops, 2)
    stage = S.SaberChainStage(chains)
    drive(comp, ops, forms + [("stage", _stage_fn(comp, stage, names, 2, x, res))])
    want = comp.eval(comp.all("A"))
    for m in ("a_0", "c3_1", "b_1"):
        set_w(ops[m], comp.B[m])
        late = S.SaberChainStage(chains)
        got = _stage_fn(comp, late, names, 2, x, res)()
        for k in names:
            same(got[k], want[k], "stage/%d built after set_weights(B) on %s: %s" % (index, m, k))
        del late


def test_chain_stage_with_tail_keeps_its_chains_first_parameters():
    import tests.test_gpu_stage_tail as TT
    assert U.TAIL_CASE == TT.TAIL_CASES[0]
    comp = U.composite("stage_tail")
    ops = _ops(comp)
    chains, names, x, res, _ = _stage_parts(comp, ops, 2)
    tail = S.SaberConvChain(ops["ha"], None, conv3x3=ops["hc3"])
    stage = S.SaberChainStage(chains, tail=tail)
    drive(comp, ops, [("stage + tail", _stage_fn(comp, stage, names, 2, x, res, "ha"))])
    set_w(ops["ha"], comp.B["ha"])
    late = S.SaberChainStage(chains, tail=tail)
    want = comp.eval(comp.all("A"))
    for k, got in _stage_fn(comp, late, names, 2, x, res, "ha")().items():
        same(got, want[k], "stage + tail built after set_weights(B) on the tail's 1x1 conv: %s" % k)


def test_xcd_stage_keeps_its_phases_first_parameters():
    comp = U.composite("xcd_stage")
    ops = _ops(comp)
    slot = {"x": 0}
    for n in comp.nodes:
        slot[n.name] = len(slot)
    stage = S.SaberStage([(ops[n.name], slot[n.src], slot[n.name], -1 if n.res is None else slot[n.res]) for n in comp.nodes])

    def fn():
        o = _outs(comp, comp.names)
        stage.dispatch([dev(comp.inputs["x"])] + [o[m] for m in comp.names])
        stage.status()
        return _host(o)
    drive(comp, ops, [("stage", fn)])


def test_stem_pair_runs_the_stem_live_and_the_pair_from_its_copy():
    """saber_hip_conv2d_stem_pair_run launches the stem op's own buffers and the pair's 1x1 convs from the object's copy: after
    set_weights(B) on the stem the pooled tensor AND both convs' outputs follow the stem; after set_weights(B) on a or b nothing changes"""
    assert U.STEM_IMAGE in P.STEM_POOL_IMAGES
    comp = U.composite("stem_pair")
    ops = _ops(comp)
    sp = S.SaberStemPair(ops["stem"], ops["a"], ops["b"])
    x = dev(comp.inputs["x"])

    def fn():
        o = _outs(comp, comp.names)
        sp.dispatch(x, o["a"], o["b"], o["stem"])
        return _host(o)
    drive(comp, ops, [("stem pair", fn)])


def test_separable_pair_keeps_its_members_first_parameters():
    comp = U.composite("sep")
    ops = _ops(comp)
    sep = S.SaberConvSep(ops["dw"], ops["pw"])
    x = dev(comp.inputs["x"])

    def form(code):
        def fn():
            sep.set_tile(code)
            o = _outs(comp, comp.names)
            sep.dispatch(x, o["pw"], o["dw"])
            return _host(o)
        return fn
    drive(comp, ops, [(("code %d" % c), form(c)) for c in _codes(sep, 15)])


@pytest.mark.parametrize("geometry", ["a", "i"])
def test_inverted_residual_block_keeps_its_members_first_parameters(geometry):
    """"a" without the residual, "i" with it: the project conv's fused eltwise (1, -0.5) reads the block's input, and out_scale_B != out_scale_A"""
    comp = U.composite("ir/" + geometry)
    assert (comp.nodes[-1].spec.mode == "elt") == (geometry == "i")
    ops = _ops(comp)
    ir = S.SaberConvIR(ops["expand"], ops["dw"], ops["project"])
    x = dev(comp.inputs["x"])

    def form(code):
        def fn():
            ir.set_tile(code)
            o = _outs(comp, comp.names)
            ir.dispatch(x, o["project"], o["expand"], o["dw"])
            return _host(o)
        return fn
    drive(comp, ops, [(("code %d" % c), form(c)) for c in _codes(ir, 7)])


def test_fire_module_keeps_its_members_first_parameters():
    comp = U.composite("fire")
    ops = _ops(comp)
    fire = S.SaberConvFire(ops["squeeze"], ops["e1"], ops["e3"])
    x = dev(comp.inputs["x"])
    e1 = comp.nodes[1].spec.geo[4]

    def form(code):
        def fn():
            fire.set_tile(code)
            w = comp.eval(comp.all("A"))
            y = blank(np.concatenate([w["e1"], w["e3"]], axis=-1))
            sq = blank(w["squeeze"])
            fire.dispatch(x, y, sq)
            got = host(y)
            return {"squeeze": host(sq), "e1": np.ascontiguousarray(got[..., :e1]), "e3": np.ascontiguousarray(got[..., e1:])}
        return fn
    drive(comp, ops, [(("code %d" % c), form(c)) for c in _codes(fire, 2)])
