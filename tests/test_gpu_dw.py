"""Depthwise 3x3 kernels (conv_dw3x3.hip; kernel selection variant 16) and MobileNet-v1 on the GPU.

INT8: every form - the static choice, the direct kernel (form 0) and each depthwise form - is bit-identical to the oracle.
FP32: every form is within the project's two 1e-4 criteria of the oracle, and every depthwise form equals form 0 bit for bit
(same operation order). MobileNet-v1 runs through the executor like ResNet50 does: every written edge and the logits bit-exact
for INT8, every produced edge within 1e-4 for FP32."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from anakin_amd import lib as L  # noqa: E402
from anakin_amd import saber as S  # noqa: E402
from anakin_amd import workloads as W  # noqa: E402
from oracle import oracle as O  # noqa: E402
from tests import dw_util as DU  # noqa: E402

FP32_RTOL = 1e-4      # tests/test_gpu_resnet.py
I8_COMBOS = [(L.U8, L.U8, True), (L.S8, L.S8, False), (L.U8, L.S8, False), (L.S8, L.U8, True), (L.U8, L.F32, False), (L.S8, L.F32, True)]
NP_DT = {L.U8: np.uint8, L.S8: np.int8, L.F32: np.float32}


def _h(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _geometries(c_choices, seed):
    """the nine MobileNet-v1 depthwise shapes at batch 1 and 8 (pad 1), then a seeded sweep of random eligible geometries"""
    geo = [(n, c, h, h, s, 1) for (c, h, s) in DU.MOBILENET_DW_SHAPES for n in (1, 8)]
    rng = np.random.default_rng(seed)
    sweep = []
    while len(sweep) < 44:
        h, w = int(rng.integers(1, 41)), int(rng.integers(1, 41))
        c, s, p, n = int(rng.choice(c_choices)), int(rng.integers(1, 3)), int(rng.integers(0, 2)), int(rng.integers(1, 6))
        if h + 2 * p < 3 or w + 2 * p < 3:      # (an empty output: not a convolution)
            continue
        sweep.append((n, c, h, w, s, p))
    return geo, sweep


def _selections(conv):
    """[(label, set_tile code or None)]: the static choice, the direct kernel, every depthwise form"""
    lib = L.load()
    assert lib.saber_hip_conv2d_get_tile(conv.h) >> 16 == 16, conv.algo()
    forms = DU.dw_forms(lib, conv.h)
    assert len(forms) >= 2, forms
    return [("static", None), ("form0", 16 << 16)] + [("form%d" % v, (16 << 16) | v) for v in forms]


def _i8_case(rng, n, c, h, w, s, p, in_dt, out_dt, relu, bias, out_scale=None):
    x = rng.integers(0, 256, (n, h, w, c)).astype(np.uint8) if in_dt == L.U8 else rng.integers(-128, 128, (n, h, w, c)).astype(np.int8)
    wt = (rng.standard_normal((c, 1, 3, 3)) * 0.4).astype(np.float32)
    b = (rng.standard_normal(c) * 0.5).astype(np.float32) if bias else None
    in_scale = 0.02
    ws = O.weight_scales(wt)
    wq = O.quant_weights(wt, ws)
    if out_scale is None:      # MAXABS scale of the op's own f32 result: nothing saturates
        bp, sc = O.conv_i8_prepare(ws, b, in_scale, 1.0, in_dt, L.F32)
        yf = O.conv_i8(x, wq, bp, sc, L.F32, relu, (p, p), (s, s), group=c)
        out_scale = max(float(np.abs(yf).max()), 1e-6) / 127.0
    bp, sc = O.conv_i8_prepare(ws, b, in_scale, out_scale, in_dt, out_dt)
    want = O.conv_i8(x, wq, bp, sc, out_dt, relu, (p, p), (s, s), group=c)
    prm = S.ConvParam(wt, b, c, (p, p), (s, s), (1, 1), relu)
    conv = S.SaberConv2D(True).init((n, c, h, w), prm, in_dt, out_dt, in_scale, out_scale, in_layout=L.NHWC, out_layout=L.NHWC)
    return conv, torch.from_numpy(x).cuda(), want, out_scale


def test_int8_every_form_bit_exact():
    """case 5: the nine MobileNet-v1 shapes at batch 1 and 8 and >= 40 random geometries, six dtype combinations, with and without
    bias: the static choice, form 0 and every depthwise form equal the oracle bit for bit - and a form v >= 1 really is a dw3x3 kernel"""
    rng = np.random.default_rng(20261)
    geo, sweep = _geometries([16, 32, 48, 80, 256, 1024], 7)
    assert len(sweep) >= 40
    ran = 0
    for i, (n, c, h, w, s, p) in enumerate(geo + sweep):
        in_dt, out_dt, relu = I8_COMBOS[0] if (i < len(geo) and i % 2 == 0) else I8_COMBOS[i % len(I8_COMBOS)]
        conv, x, want, _ = _i8_case(rng, n, c, h, w, s, p, in_dt, out_dt, relu, bias=bool(i % 3))
        for label, code in _selections(conv):
            if code is not None:
                conv.set_tile(code)
            if label not in ("static", "form0"):
                assert conv.algo().startswith("dw3x3_i8_"), (label, conv.algo())
            if label == "form0":
                assert conv.algo() == "direct_i8"
            y = conv.new_output()
            y.fill_(77)
            conv.dispatch(x, y)
            assert np.array_equal(_h(y), want), ((n, c, h, w, s, p), (in_dt, out_dt, relu), label, conv.algo())
        ran += 1
    assert ran == len(geo) + len(sweep) == 18 + 44


@pytest.mark.parametrize("out_dt", [L.U8, L.S8])
def test_int8_saturation(out_dt):
    """case 6: out_scale = a quarter of the MAXABS scale - the oracle output holds saturated and unsaturated values, every form equals it"""
    rng = np.random.default_rng(20262 + out_dt)
    hi, lo = (255, 0) if out_dt == L.U8 else (127, -128)
    for (n, c, h, w, s, p), in_dt, relu in (((2, 32, 28, 28, 1, 1), L.U8, True), ((1, 64, 15, 9, 2, 1), L.S8, False),
                                            ((3, 256, 7, 7, 1, 1), L.U8, False), ((1, 16, 33, 20, 2, 0), L.S8, True)):
        seed = int(rng.integers(1 << 30))
        _, _, _, scale = _i8_case(np.random.default_rng(seed), n, c, h, w, s, p, in_dt, out_dt, relu, True)
        # the same operands again (same generator state: same x, same weights) with a quarter of that scale
        conv, x, want, _ = _i8_case(np.random.default_rng(seed), n, c, h, w, s, p, in_dt, out_dt, relu, True, out_scale=scale / 4)
        sat = np.count_nonzero(want == hi) + (0 if (relu or out_dt == L.U8) else np.count_nonzero(want == lo))
        assert 0 < sat < want.size and np.count_nonzero((want > lo) & (want < hi)) > 0, (sat, want.size)
        for label, code in _selections(conv):
            if code is not None:
                conv.set_tile(code)
            y = conv.new_output()
            conv.dispatch(x, y)
            assert np.array_equal(_h(y), want), ((n, c, h, w, s, p), label, conv.algo())


def _fp32_close(got_nhwc, want_nchw, what):
    got = got_nhwc.transpose(0, 3, 1, 2)
    d = np.abs(got - want_nchw)
    e_max = float(d.max() / max(np.abs(want_nchw).max(), 1e-30))
    e_el = float((d / (np.abs(want_nchw) + np.abs(want_nchw).mean() + 1e-30)).max())
    assert e_max <= FP32_RTOL and e_el <= FP32_RTOL, (what, e_max, e_el)
    return e_max, e_el


def test_fp32_every_form():
    """case 7: the same shapes and sweep (C % 4 == 0), relu / none / leaky 0.1: every form within the two 1e-4 criteria of the oracle,
    every depthwise form bit-identical to form 0"""
    rng = np.random.default_rng(20263)
    geo, sweep = _geometries([4, 12, 32, 48, 80, 256, 1024], 11)
    worst = (0.0, 0.0)
    for i, (n, c, h, w, s, p) in enumerate(geo + sweep):
        act = ("relu", "none", "leaky")[i % 3]
        x = rng.standard_normal((n, c, h, w)).astype(np.float32)
        wt = (rng.standard_normal((c, 1, 3, 3)) * np.sqrt(2.0 / 9)).astype(np.float32)
        b = (rng.standard_normal(c) * 0.3).astype(np.float32) if i % 4 else None
        want = O.conv_f32_nchw(x, wt, b, act == "relu", (p, p), (s, s), group=c)
        if act == "leaky":
            want = np.where(want > 0, want, want * np.float32(0.1)).astype(np.float32)
        prm = S.ConvParam(wt, b, c, (p, p), (s, s), (1, 1), act != "none")
        prm.negative_slope = 0.1 if act == "leaky" else 0.0
        conv = S.SaberConv2D(False).init((n, c, h, w), prm, L.F32, L.F32, in_layout=L.NHWC, out_layout=L.NHWC)
        xd = torch.from_numpy(np.ascontiguousarray(x.transpose(0, 2, 3, 1))).cuda()
        base = None
        for label, code in _selections(conv)[1:] + [("static", None)]:      # form 0 first: the others are compared with it
            if code is not None:
                conv.set_tile(code)
            if label.startswith("form") and label != "form0":
                assert conv.algo().startswith("dw3x3_f32_"), (label, conv.algo())
            y = conv.new_output()
            y.fill_(7.0)
            conv.dispatch(xd, y)
            got = _h(y)
            e = _fp32_close(got, want, ((n, c, h, w, s, p), act, label, conv.algo()))
            worst = (max(worst[0], e[0]), max(worst[1], e[1]))
            if label == "form0":
                assert conv.algo() == "direct_f32"
                base = got
            elif label != "static":
                assert np.array_equal(got, base), ((n, c, h, w, s, p), act, label)
    print("FP32 depthwise: %d geometries, worst max-norm %.2e, worst element-wise %.2e" % (len(geo) + len(sweep), worst[0], worst[1]))


@pytest.mark.parametrize("int8", [True, False])
def test_set_weights_twice_on_a_live_op(int8):
    """case 8: saber_hip_conv2d_set_weights again on a live op: the second weights and bias run (the [tap][C] packing follows), the
    selection stays"""
    rng = np.random.default_rng(20264)
    n, c, h, s, p = 2, 64, 19, 1, 1
    lib = L.load()
    for v in (1, 2):
        w1, w2 = [(rng.standard_normal((c, 1, 3, 3)) * 0.4).astype(np.float32) for _ in range(2)]
        b1, b2 = [(rng.standard_normal(c) * 0.5).astype(np.float32) for _ in range(2)]
        if int8:
            x = rng.integers(0, 256, (n, h, h, c)).astype(np.uint8)
            conv = S.SaberConv2D(True).init((n, c, h, h), S.ConvParam(w1, b1, c, (p, p), (s, s), (1, 1), True), L.U8, L.U8, 0.02, 0.11,
                                            in_layout=L.NHWC, out_layout=L.NHWC)
            ws = O.weight_scales(w2)
            bp, sc = O.conv_i8_prepare(ws, b2, 0.03, 0.09, L.U8, L.U8)
            want = O.conv_i8(x, O.quant_weights(w2, ws), bp, sc, L.U8, True, (p, p), (s, s), group=c)
            xd = torch.from_numpy(x).cuda()
        else:
            x = rng.standard_normal((n, c, h, h)).astype(np.float32)
            conv = S.SaberConv2D(False).init((n, c, h, h), S.ConvParam(w1, b1, c, (p, p), (s, s), (1, 1), True), L.F32, L.F32,
                                             in_layout=L.NHWC, out_layout=L.NHWC)
            want = O.conv_f32_nchw(x, w2, b2, True, (p, p), (s, s), group=c)
            xd = torch.from_numpy(np.ascontiguousarray(x.transpose(0, 2, 3, 1))).cuda()
        conv.set_tile((16 << 16) | v)
        y = conv.new_output()
        conv.dispatch(xd, y)
        first = _h(y).copy()
        conv.set_weights(w2, b2, None, 0.03, 0.09)
        assert lib.saber_hip_conv2d_get_tile(conv.h) == (16 << 16) | v
        assert conv.algo().startswith("dw3x3_")
        conv.dispatch(xd, y)
        got = _h(y)
        assert not np.array_equal(got, first)
        if int8:
            assert np.array_equal(got, want)
        else:
            _fp32_close(got, want, ("set_weights twice", v))


def _dw_ops(net):
    return [i for i, c in enumerate(net.choices()) if (c >> 16) & 0xff == 16]


def _force(net, v):
    ch = net.choices()
    idx = [i for i, c in enumerate(ch) if (c >> 16) & 0xff == 16]
    assert len(idx) == 13, idx
    for i in idx:
        ch[i] = (16 << 16) | v
    net.set_choices(ch)
    return idx


@pytest.fixture(scope="module")
def mobilenet():
    L.require_device()
    model = W.build_model("mobilenet_v1")
    fw = W.framework_model(model, "int8")
    cache = {}

    def at(batch):
        if batch not in cache:
            x = W.make_input(batch)
            scales = W.calibrate(model, x)
            cache[batch] = (x, scales, DU.run_int8(fw, scales, x))
        return cache[batch]
    return model, fw, at


def _check_int8_net(net, x, ref, what):
    def compare():
        torch.cuda.synchronize()
        checked = 0
        for name in net.tensors:
            if name == "data" or name not in ref or net.unwritten(name):
                continue
            got, want = _h(net.tensor(name)), ref[name]
            if name == "prob":
                assert np.abs(got - want.reshape(got.shape)).max() <= 1e-4 * want.max(), (what, name)
            else:
                assert np.array_equal(got, want.reshape(got.shape)), (what, name)
            checked += 1
        assert checked >= 30, (what, checked)      # 27 conv edges (all written: MobileNet has no chain), pool6, fc7, prob
    xd = torch.from_numpy(x).cuda()
    net.tensor("data").copy_(xd)
    net.run()
    compare()
    net.tensor("fc7").zero_()
    net.capture()
    net.replay()
    compare()
    net.autotune(iters=2)
    net.tensor("data").copy_(xd)
    net.run()
    compare()


@pytest.mark.parametrize("fuse", [False, True])
def test_mobilenet_v1_int8_every_edge_bit_exact(mobilenet, fuse):
    """case 9: MobileNet-v1 INT8 (the framework's op list: every edge u8, u8 average pooling, fc with a u8 operand) at batch 1, 2, 8 -
    unfused and with the default fusions; eager, replayed, autotuned; with the static selection and with every depthwise form forced
    on the 13 depthwise ops; image 0 of batch 8 equals batch 1"""
    model, fw, at = mobilenet
    for batch in (1, 2, 8):
        x, scales, ref = at(batch)
        probe = W.build_int8_net(fw, dict(scales), batch, fuse=fuse)
        forms = DU.dw_forms(L.load(), probe.keep[1].h)      # (keep[1]: conv2_dw)
        assert len(forms) >= 2
        for v in [None] + forms:
            net = probe if v is None else W.build_int8_net(fw, dict(scales), batch, fuse=fuse)
            if v is not None:
                idx = _force(net, v)
                assert sum(1 for i in idx if "dw3x3_i8_" in net.op_name(i)) == 13, [net.op_name(i) for i in idx]
            else:
                assert len(_dw_ops(net)) == 13
            _check_int8_net(net, x, ref, (batch, fuse, v))
    # batch invariance with ONE set of scales: image 0 of the batch of 8 against the same image alone, on the device and in the oracle
    x8, s8, ref8 = at(8)
    n8 = W.build_int8_net(fw, dict(s8), 8, fuse=fuse)
    n1 = W.build_int8_net(fw, dict(s8), 1, fuse=fuse)
    n8.tensor("data").copy_(torch.from_numpy(x8).cuda())
    n1.tensor("data").copy_(torch.from_numpy(x8[:1]).cuda())
    n8.run()
    n1.run()
    assert np.array_equal(_h(n8.tensor("fc7"))[0], _h(n1.tensor("fc7"))[0])
    assert np.array_equal(_h(n1.tensor("fc7"))[0], ref8["fc7"][0])


def _fp32_net_edges(net, x, ref, what):
    net.tensor("data").copy_(torch.from_numpy(x).cuda())
    done, checked = -1, 0
    for idx, name in net.produced:
        while done < idx:
            done += 1
            net.run_op(done)
        got = _h(net.tensor(net.alias.get(name, name)))
        want = ref[name]
        got = got.transpose(0, 3, 1, 2) if got.ndim == 4 else got.reshape(want.reshape(got.shape[0], -1).shape)
        want = want.reshape(got.shape)
        d = np.abs(got - want)
        e_max = float(d.max() / np.abs(want).max())
        e_el = float((d / (np.abs(want) + np.abs(want).mean())).max())
        assert e_max <= FP32_RTOL and e_el <= FP32_RTOL, (what, name, e_max, e_el)
        checked += 1
    assert done == net.num_ops() - 1
    return checked


def test_mobilenet_v1_fp32_every_edge():
    """case 10: MobileNet-v1 FP32 at batch 1 and 8: every produced edge within the two 1e-4 criteria, with the static selection and with
    each depthwise form forced on the 13 depthwise ops; two reproducible nets, autotuned, answer with the same bits"""
    L.require_device()
    model = W.build_model("mobilenet_v1")
    for batch in (1, 8):
        x = W.make_input(batch)
        ref = DU.run_fp32(model, x)
        probe = W.build_fp32_net(model, batch)
        dw = _dw_ops(probe)
        assert len(dw) == 13
        forms = DU.dw_forms(L.load(), next(k for k in probe.keep if getattr(getattr(k, "desc", None), "group", 1) > 1).h)
        for v in [None] + forms:
            net = probe if v is None else W.build_fp32_net(model, batch)
            if v is not None:
                idx = _force(net, v)
                assert sum(1 for i in idx if "dw3x3_f32_" in net.op_name(i)) == 13, [net.op_name(i) for i in idx]
            assert _fp32_net_edges(net, x, ref, (batch, v)) >= 30
    x = W.make_input(2)
    outs = []
    for _ in range(2):
        net = W.build_fp32_net(model, 2, reproducible=True)
        static_names = [net.op_name(k) for k in range(net.num_ops())]
        net.tensor("data").copy_(torch.from_numpy(x).cuda())
        net.run()
        net.autotune(iters=2)
        assert [net.op_name(k) for k in range(net.num_ops())] == static_names
        net.tensor("data").copy_(torch.from_numpy(x).cuda())
        net.run()
        outs.append({n: _h(net.tensor(n)).copy() for n in ("fc7", "prob", "conv2_dw", "conv14_dw")})
    for n in outs[0]:
        assert np.array_equal(outs[0][n], outs[1][n]), n


def test_op_work_of_a_depthwise_op(mobilenet):
    """case 11: saber_hip_net_op_work divides by `group`: 2 * 9 * C * oh * ow * n operations, in + out + 9 * C elements"""
    model, fw, at = mobilenet
    x, scales, _ = at(2)
    net = W.build_int8_net(fw, dict(scales), 2, fuse=False)
    spec = [l for l in fw["spec"] if l["kind"] == "conv"]
    hw, seen = 224, 0
    for i, l in enumerate(spec):      # (unfused: op i is conv i)
        ho = (hw + 2 * l["pad"] - l["k"]) // l["stride"] + 1
        if l.get("group", 1) > 1:
            c = l["cin"]
            by, fl = net.op_work(i)
            assert fl == 2 * 9 * c * ho * ho * 2, (l["name"], fl)
            assert by == 2 * hw * hw * c + 2 * ho * ho * c + 9 * c, (l["name"], by)
            seen += 1
        hw = ho
    assert seen == 13
    fnet = W.build_fp32_net(model, 2)
    i = _dw_ops(fnet)[0]      # conv2_dw: 32 channels, 112 x 112, stride 1
    by, fl = fnet.op_work(i)
    assert fl == 2 * 9 * 32 * 112 * 112 * 2 and by == 4 * (2 * 2 * 112 * 112 * 32 + 9 * 32), (by, fl)
