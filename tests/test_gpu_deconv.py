"""The deconv op on the GPU (anakin_amd/csrc/deconv.hip): every form on the smallest shapes at which each mechanism can fail - more than one
cell tile along x among them - against the float64 scatter of tests/deconv_util.py; single-term probes at 4 u and guard bands, across a
column seam too; a seeded random-geometry sweep of every form; form 0 beyond one grid stride; set_weights on a live op; the op inside the executor (an
encoder - decoder list with a skip connection); the Saber-side class through the stand-in C++ driver."""
import os
import subprocess

import numpy as np
import pytest
import torch

from anakin_amd import lib as L
from anakin_amd import saber as S
from oracle import oracle as O
from tests import deconv_util as DU
from tests import fp32_probe as FP
from tests import guard_util as GU

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["deconv_direct_f32", "deconv_b3_f32_4x16", "deconv_b3_f32_2x16"]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def nhwc(a):
    return np.ascontiguousarray(a.transpose(0, 2, 3, 1))


def _op(cs, w, b, relu=False, in_layout=L.NHWC, out_layout=L.NHWC):
    p = S.ConvParam(w, b, cs["group"], cs["pad"], cs["stride"], cs["dil"], relu)
    return S.SaberDeconv2D().init((cs["n"], cs["c"], cs["h"], cs["w"]), p, in_layout, out_layout)


def _run(op, x_nchw, form):
    """the op's output as NCHW, whatever its layouts"""
    op.set_tile(form)
    assert op.algo() == NAMES[form] and op.tile() == form
    x = dev(x_nchw if op.desc.in_layout == L.NCHW else nhwc(x_nchw))
    y = op.new_output()
    y.fill_(float("nan"))
    op.dispatch(x, y)
    got = host(y)
    return got if op.desc.out_layout == L.NCHW else got.transpose(0, 3, 1, 2)


@pytest.mark.parametrize("name", sorted(DU.ALL_CASES))
def test_every_form_with_and_without_bias_and_relu(name):
    """every accepted form within the project's two 1e-4 criteria of the float64 rule; the bf16-plane forms bit-identical to each other"""
    cs = DU.ALL_CASES[name]
    x, w, b = DU.make(cs, np.random.default_rng(FP._seed(name)))
    for bias in (b, None):
        for relu in (False, True):
            op = _op(cs, w, bias, relu)
            forms = op.forms()
            assert forms == ([0, 1, 2] if name in DU.B3_CASES else [0]), (name, forms)
            want = DU.deconv_ref(x, w, bias, cs, relu)
            got = {f: _run(op, x, f) for f in forms}
            for f in forms:
                assert got[f].shape == want.shape
                DU.fp32_close(got[f], want, (name, NAMES[f], bias is not None, relu))
            if len(forms) == 3:
                assert GU.same_bytes(got[1], got[2]), (name, "the two bf16-plane forms differ")


@pytest.mark.parametrize("in_layout,out_layout", [(L.NHWC, L.NHWC), (L.NHWC, L.NCHW), (L.NCHW, L.NHWC), (L.NCHW, L.NCHW)])
def test_direct_kernel_in_all_four_layout_combinations(in_layout, out_layout):
    for name in ("group2", "k2x3_s2x1_p0x1", "k4s2p1"):
        cs = DU.ALL_CASES[name]
        x, w, b = DU.make(cs, np.random.default_rng(FP._seed(name) + 1))
        op = _op(cs, w, b, True, in_layout, out_layout)
        assert op.forms() == ([0, 1, 2] if (name == "k4s2p1" and in_layout == out_layout == L.NHWC) else [0])
        DU.fp32_close(_run(op, x, 0), DU.deconv_ref(x, w, b, cs, True), (name, in_layout, out_layout))


@pytest.mark.parametrize("name", DU.PROBE_CASES)
def test_single_term_probes(name):
    """weight and activation probes, every form, bound fp32_probe.BOUND_U, full coverage asserted"""
    cs = DU.B3_CASES[name]
    pr = DU.build_probes(name)
    wpasses, wcov, reach = pr["weight"]
    apasses, xcov, poscov, xread = pr["activation"]
    assert (wcov | ~reach).all() and reach.all() and poscov.all() and np.array_equal(xcov, xread) and xread.all()
    op = _op(cs, wpasses[0].w, wpasses[0].bias)
    for p in wpasses:
        for f in (0, 1, 2):
            p.check(_run(op, p.x, f), "%s weight probe, %s" % (name, NAMES[f]))
    for p in apasses:
        op.set_weights(p.w, p.bias)      # a live op: every packing follows
        for f in (0, 1, 2):
            p.check(_run(op, p.x, f), "%s activation probe, %s" % (name, NAMES[f]))


@pytest.mark.parametrize("name", ["k4s2p1", "k3s2p0", "ragged", "k2s2p0", "depthwise_k4s2p1", "k5s3p1", "seam_k4p1_probe", "seam_k3p1_probe"])
def test_every_form_between_guard_bands(name):
    """nothing is written outside the output, the read-only tensors keep their bytes, and the output does not depend on what lies next
    to the tensors (tests/guard_util.py)"""
    cs = DU.ALL_CASES[name]
    x, w, b = DU.make(cs, np.random.default_rng(FP._seed(name) + 2))
    op = _op(cs, w, b, True)
    want = DU.deconv_ref(x, w, b, cs, True)
    oh, ow = DU.out_hw(cs)

    def plain(inputs, outputs, ws_bytes):
        T = {n: dev(a) for n, a in inputs.items()}
        for n, (shape, dt, prev) in outputs.items():
            T[n] = torch.full(shape, float(GU.SENTINEL), dtype=torch.float32, device="cuda")
        return T, None

    for f in op.forms():
        op.set_tile(f)
        out = GU.run_guarded({"x": nhwc(x)}, {"y": ((cs["n"], oh, ow, cs["k"]), np.float32, None)},
                             lambda T, ws: op.dispatch(T["x"], T["y"]), plain=plain, what="%s %s" % (name, NAMES[f]))
        GU.assert_no_sentinel_run(out["y"], "%s %s" % (name, NAMES[f]))
        DU.fp32_close(out["y"].transpose(0, 3, 1, 2), want, (name, NAMES[f]))


@pytest.mark.parametrize("seed", DU.SWEEP_SEEDS)
def test_random_geometry_sweep_of_every_form(seed):
    """deconv_util.sweep_draws (the class drawn first, then the shape; tests/test_deconv_cpu.py asserts what the seeds cover): the direct
    kernel over groups, kh != kw, per-axis stride / dilation / pad, ragged channels and the four layout pairs; the bf16-plane forms over
    k, unequal pads and one to three cell tiles each way - every form against the float64 rule, forms 1 and 2 byte for byte. No draw is
    left out."""
    draws = DU.sweep_draws(seed)
    ran = 0
    for d in draws["direct"]:
        cs = d["cs"]
        x, w, b = DU.make(cs, np.random.default_rng(seed), bias=d["bias"])
        op = _op(cs, w, b, d["relu"], L.NCHW if d["in_nchw"] else L.NHWC, L.NCHW if d["out_nchw"] else L.NHWC)
        assert op.forms() == [0], cs
        DU.fp32_close(_run(op, x, 0), DU.deconv_ref(x, w, b, cs, d["relu"]), (seed, d))
        ran += 1
    for d in draws["b3"]:
        cs = d["cs"]
        x, w, b = DU.make(cs, np.random.default_rng(seed), bias=d["bias"])
        op = _op(cs, w, b, d["relu"])
        assert op.forms() == [0, 1, 2], cs
        want = DU.deconv_ref(x, w, b, cs, d["relu"])
        got = [_run(op, x, f) for f in (0, 1, 2)]
        for f in (0, 1, 2):
            DU.fp32_close(got[f], want, (seed, NAMES[f], d))
        assert GU.same_bytes(got[1], got[2]), (seed, d, "the two bf16-plane forms differ")
        ran += 1
    assert ran == DU.SWEEP_DIRECT + DU.SWEEP_B3


@pytest.mark.parametrize("out_layout", [L.NHWC, L.NCHW])
def test_direct_kernel_beyond_one_grid_stride(out_layout):
    """4 259 840 outputs against a grid capped at 16 384 blocks of 256 lanes: the loop's second trip, under both index decompositions"""
    cs = DU.STRIDE_CASES["two_grid_strides"]
    x, w, b = DU.make(cs, np.random.default_rng(FP._seed("two_grid_strides")))
    op = _op(cs, w, b, False, L.NHWC, out_layout)
    assert op.forms() == [0]
    DU.fp32_close(_run(op, x, 0), DU.deconv_ref(x, w, b, cs), ("two grid strides", out_layout))


def test_set_weights_twice_on_a_live_op():
    """the second weights and bias reach every form (no stale planes), a bias can go and come back, the selection stays"""
    cs = DU.B3_CASES["k4s2p1"]
    rng = np.random.default_rng(5)
    x, w1, b1 = DU.make(cs, rng)
    _, w2, b2 = DU.make(cs, rng)
    op = _op(cs, w1, b1)
    for f in (2, 0, 1):
        op.set_tile(f)
        first = _run(op, x, f)
        DU.fp32_close(first, DU.deconv_ref(x, w1, b1, cs), ("first", f))
        op.set_weights(w2, None)
        assert op.tile() == f and op.algo() == NAMES[f]
        DU.fp32_close(_run(op, x, f), DU.deconv_ref(x, w2, None, cs), ("second, no bias", f))
        for g in (0, 1, 2):
            DU.fp32_close(_run(op, x, g), DU.deconv_ref(x, w2, None, cs), ("second, other form", f, g))
        op.set_weights(w1, b1)
        assert GU.same_bytes(_run(op, x, f), first), ("back to the first weights", f)


# ---- the op inside the executor -------------------------------------------------------------------------------------------------------------
def _conv(shape, w, b, pad, relu):
    p = S.ConvParam(w, b, 1, (pad, pad), (1, 1), (1, 1), relu)
    return S.SaberConv2D(False).init(shape, p, L.F32, L.F32, in_layout=L.NHWC, out_layout=L.NHWC)


def _encoder_decoder(flags=0):
    """conv3x3 -> max pooling 2x2 -> conv3x3 -> deconv k2 s2 -> concat with the skip -> conv3x3 -> conv1x1, 12 x 10 image, batch 2, NHWC f32"""
    n, h, w, c0, c1, c2, kout = 2, 12, 10, 4, 16, 32, 8
    rng = np.random.default_rng(77)
    x = rng.standard_normal((n, c0, h, w)).astype(np.float32)

    def wb(k, c, ks):
        return (rng.standard_normal((k, c, ks, ks)) * (1.0 / np.sqrt(c * ks * ks))).astype(np.float32), (rng.standard_normal(k) * 0.1).astype(np.float32)
    (w_e1, b_e1), (w_e2, b_e2), (w_d1, b_d1), (w_o, b_o) = wb(c1, c0, 3), wb(c2, c1, 3), wb(c1, 2 * c1, 3), wb(kout, c1, 1)
    w_up = (rng.standard_normal((c2, c1, 2, 2)) * 0.2).astype(np.float32)
    b_up = (rng.standard_normal(c1) * 0.1).astype(np.float32)
    cs = DU.case(n, h // 2, w // 2, c2, c1, 2)
    ref = {"x": x}
    ref["e1"] = O.conv_f32_nchw(x, w_e1, b_e1, True, (1, 1))
    ref["p1"] = O.pool_f32_nchw(ref["e1"], (2, 2), (2, 2), (0, 0), 0)
    ref["e2"] = O.conv_f32_nchw(ref["p1"], w_e2, b_e2, True, (1, 1))
    ref["up"] = DU.deconv_ref(ref["e2"], w_up, b_up, cs, True).astype(np.float32)
    ref["cat"] = np.concatenate([ref["up"], ref["e1"]], 1)
    ref["d1"] = O.conv_f32_nchw(ref["cat"], w_d1, b_d1, True, (1, 1))
    ref["out"] = O.conv_f32_nchw(ref["d1"], w_o, b_o, False)
    net = S.Net()
    for nm in ref:
        nn, cc, hh, ww = ref[nm].shape
        net.add_tensor(nm, (nn, hh, ww, cc), L.F32)
    net.add_conv(_conv((n, c0, h, w), w_e1, b_e1, 1, True), "x", "e1")
    net.add_pool_f32(n, h, w, c1, h // 2, w // 2, (2, 2), (2, 2), (0, 0), L.POOL_MAX, L.NHWC, "e1", "p1")
    net.add_conv(_conv((n, c1, h // 2, w // 2), w_e2, b_e2, 1, True), "p1", "e2")
    up = S.SaberDeconv2D().init((n, c2, h // 2, w // 2), S.ConvParam(w_up, b_up, 1, (0, 0), (2, 2), (1, 1), True))
    i_up = net.add_deconv(up, "e2", "up")
    net.add_concat(["up", "e1"], "cat")
    net.add_conv(_conv((n, 2 * c1, h, w), w_d1, b_d1, 1, True), "cat", "d1")
    net.add_conv(_conv((n, c1, h, w), w_o, b_o, 0, False), "d1", "out")
    if flags:
        net.optimize(flags)
    net.finalize()
    return net, ref, i_up, up


def _check_edges(net, ref, what, names=None):
    for nm in (names or [k for k in ref if k != "x"]):
        DU.fp32_close(host(net.tensor(nm)).transpose(0, 3, 1, 2), ref[nm], (what, nm))


def _fill(net, ref):
    for nm in ref:
        net.tensor(nm).fill_(float("nan"))
    net.tensor("x").copy_(dev(nhwc(ref["x"])))


def test_encoder_decoder_list_eager_replayed_and_autotuned():
    net, ref, i_up, up = _encoder_decoder()
    assert net.op_name(i_up) == "deconv:" + up.algo() and net.num_ops() == net.num_launches() == 7
    cs = up.desc
    nbytes, flops = net.op_work(i_up)
    wel = cs.c * cs.k * cs.kh * cs.kw
    assert nbytes == 4.0 * (ref["e2"].size + ref["up"].size + wel) and flops == 2.0 * cs.n * cs.h * cs.w * wel
    _fill(net, ref)
    net.run()
    _check_edges(net, ref, "eager")
    _fill(net, ref)
    net.capture()
    net.replay()
    _check_edges(net, ref, "replayed")
    # one op on its own; every form through the choice word
    for form in (1, 2, 0):
        ch = net.choices()
        assert ch[i_up] >> 16 == 18
        ch[i_up] = (18 << 16) | form
        net.set_choices(ch)
        assert net.choices()[i_up] == (18 << 16) | form and net.op_name(i_up) == "deconv:" + NAMES[form]
        net.tensor("up").fill_(float("nan"))
        net.run_op(i_up)
        _check_edges(net, ref, "run_op form %d" % form, ["up"])
    ch = net.choices()
    ch[i_up] = (18 << 16) | 7
    with pytest.raises(L.SaberHipError):
        net.set_choices(ch)
    assert net.op_name(i_up) == "deconv:" + NAMES[0]
    # the autotuner times every accepted form at the site; its choice round-trips
    _fill(net, ref)
    net.run()
    net.autotune(5)
    tuned = net.choices()
    assert tuned[i_up] >> 16 == 18 and (tuned[i_up] & 0xffff) in (0, 1, 2)
    names = [net.op_name(i) for i in range(net.num_ops())]
    assert names[i_up] == "deconv:" + NAMES[tuned[i_up] & 0xffff]
    _fill(net, ref)
    net.capture()
    net.replay()
    _check_edges(net, ref, "autotuned, replayed")
    net2, _, _, _ = _encoder_decoder()
    net2.set_choices(tuned)
    assert [net2.op_name(i) for i in range(net2.num_ops())] == names
    _fill(net2, ref)
    net2.run()
    _check_edges(net2, ref, "restored selection")


def test_two_reproducible_nets_are_bit_identical_and_the_arena_compacts():
    outs = []
    for k in range(2):
        net, ref, i_up, up = _encoder_decoder(8192)      # SABER_HIP_NET_REPRODUCIBLE_FP32
        before = [net.op_name(i) for i in range(net.num_ops())]
        _fill(net, ref)
        net.run()
        net.autotune(3)
        assert [net.op_name(i) for i in range(net.num_ops())] == before, "an FP32 op moved in reproducible mode"
        ch = net.choices()
        ch[i_up] = (18 << 16) | 1
        net.set_choices(ch)      # a restored selection does not move it either
        assert net.op_name(i_up) == before[i_up]
        full = net.arena_bytes()
        net.compact()
        assert net.compacted() and net.arena_bytes() < full
        net.tensor("x").copy_(dev(nhwc(ref["x"])))
        net.run()
        _check_edges(net, ref, "compacted", ["out"])
        outs.append(host(net.tensor("out")).copy())
    assert GU.same_bytes(outs[0], outs[1])


def test_deconv_is_recorded_by_the_op_list_capture():
    cs = DU.B3_CASES["k3s2p1"]
    x, w, b = DU.make(cs, np.random.default_rng(9))
    op = _op(cs, w, b)
    xd, y = dev(nhwc(x)), op.new_output()
    y.fill_(123.0)
    with S.Capture() as cap:
        op.dispatch(xd, y)
    assert float(host(y).min()) == 123.0 == float(host(y).max())      # recorded, not launched
    net = cap.net
    assert net.num_ops() == 1 and net.op_name(0) == "deconv:" + op.algo()
    net.bind(net.tensor_of_ptr(y), y)
    net.finalize()
    net.run()
    DU.fp32_close(host(y).transpose(0, 3, 1, 2), DU.deconv_ref(x, w, b, cs), "captured list")


def test_saber_deconv_through_the_stand_in_cpp_driver():
    """tests/cpp/test_saber_deconv.cpp: SaberDeconv2D<MI355X, AK_FLOAT> init -> dispatch under the stand-in Saber headers"""
    exe = os.path.join(ROOT, "tests", "cpp", "test_saber_deconv.bin")
    assert os.path.exists(exe), "tests/cpp/test_saber_deconv.bin is missing: run __graft_entry__.build()"
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = os.pathsep.join([os.path.join(ROOT, "anakin_amd"), os.path.join(ROOT, "oracle"), env.get("LD_LIBRARY_PATH", "")])
    p = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0 and "deconv cases within 1e-4" in p.stdout, p.stdout[-3000:] + p.stderr[-2000:]
