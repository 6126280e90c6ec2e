"""Grouped 3x3 INT8 kernels (conv_group3x3.hip; kernel selection variant 17) and ResNeXt-50 32x4d on the GPU.

Every form - the static choice, the direct kernel (form 0) and each matrix-core form - is bit-identical to the oracle, whose grouped
INT8 convolution is pinned to the reference's (tests/test_oracle_vs_ref.py). ResNeXt-50 runs through the executor like ResNet50 does:
every written edge and the logits bit-exact for INT8, every produced edge within 1e-4 for FP32 (grouped FP32 layers stay on the direct
kernel)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from anakin_amd import lib as L  # noqa: E402
from anakin_amd import saber as S  # noqa: E402
from anakin_amd import workloads as W  # noqa: E402
from oracle import oracle as O  # noqa: E402
from tests import dw_util as DU  # noqa: E402
from tests import group_util as GU  # noqa: E402
from tests import int8_probe as P  # noqa: E402
from tests.test_gpu_dw import FP32_RTOL, I8_COMBOS  # noqa: E402

V = GU.VARIANT
SENTINEL = 77


def _h(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _selections(conv):
    """[(label, set_tile code or None)]: the static choice, the direct kernel, every grouped form"""
    lib = L.load()
    assert lib.saber_hip_conv2d_get_tile(conv.h) >> 16 == V, conv.algo()
    forms = GU.group_forms(lib, conv.h)
    assert len(forms) >= 1, forms
    return [("static", None), ("form0", V << 16)] + [("form%d" % v, (V << 16) | v) for v in forms]


def _every_form(conv, x, want, what):
    """runs every selection of `conv` on x into a sentinel-filled output and compares with `want` bit for bit"""
    names = []
    for label, code in _selections(conv):
        if code is not None:
            conv.set_tile(code)
        if label == "form0":
            assert conv.algo() == "direct_i8"
        elif label != "static":
            assert conv.algo().startswith("g3x3_i8_"), (label, conv.algo())
        y = conv.new_output()
        y.fill_(SENTINEL)
        conv.dispatch(x, y)
        got = _h(y)
        assert np.array_equal(got, want), (what, label, conv.algo(), int(np.count_nonzero(got != want)))
        names.append(conv.algo())
    return names


def _i8_case(rng, n, c, cg, h, w, s, p, in_dt, out_dt, relu, bias, out_scale=None):
    x = rng.integers(0, 256, (n, h, w, c)).astype(np.uint8) if in_dt == L.U8 else rng.integers(-128, 128, (n, h, w, c)).astype(np.int8)
    wt = (rng.standard_normal((c, cg, 3, 3)) * 0.4).astype(np.float32)
    b = (rng.standard_normal(c) * 0.5).astype(np.float32) if bias else None
    in_scale = 0.02
    ws = O.weight_scales(wt)
    wq = O.quant_weights(wt, ws)
    g = c // cg
    if out_scale is None:      # MAXABS scale of the op's own f32 result: nothing saturates
        bp, sc = O.conv_i8_prepare(ws, b, in_scale, 1.0, in_dt, L.F32)
        yf = O.conv_i8(x, wq, bp, sc, L.F32, relu, (p, p), (s, s), group=g)
        out_scale = max(float(np.abs(yf).max()), 1e-6) / 127.0
    bp, sc = O.conv_i8_prepare(ws, b, in_scale, out_scale, in_dt, out_dt)
    want = O.conv_i8(x, wq, bp, sc, out_dt, relu, (p, p), (s, s), group=g)
    prm = S.ConvParam(wt, b, g, (p, p), (s, s), (1, 1), relu)
    conv = S.SaberConv2D(True).init((n, c, h, w), prm, in_dt, out_dt, in_scale, out_scale, in_layout=L.NHWC, out_layout=L.NHWC)
    return conv, torch.from_numpy(x).cuda(), want, out_scale


def _sweep(seed):
    """three draws for every (C, Cg) with C in {64, 128, 192, 320} and Cg | C a grouped conv: H, W in 1 .. 23 independently, n in 1 .. 3,
    stride 1 | 2, pad 0 | 1; then the fixed corner cases (1 x 1 with pad 1, one ragged tile, exactly one and exactly four full tiles)"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(3):
        for c in (64, 128, 192, 320):
            for cg in GU.CGS:
                if c % cg or cg == c:
                    continue
                out.append((int(rng.integers(1, 4)), c, cg, int(rng.integers(1, 24)), int(rng.integers(1, 24)), int(rng.integers(1, 3)),
                            int(rng.integers(0, 2))))
    out += [(1, 64, 4, 1, 1, 1, 1), (3, 128, 64, 1, 1, 2, 1), (1, 64, 32, 1, 17, 1, 1), (1, 64, 16, 4, 4, 1, 1), (1, 128, 8, 8, 8, 1, 1),
            (2, 192, 64, 5, 13, 2, 0)]
    return out


def test_int8_every_form_bit_exact():
    """test 3: the seven ResNeXt-50 shapes at batch 1, two of them at batch 8, and a seeded sweep of small geometries; the six dtype /
    relu combinations, with and without bias; the output pre-filled with a sentinel"""
    rng = np.random.default_rng(20271)
    geo = [(1, c, cg, h, h, s, 1) for (c, cg, h, s) in GU.RESNEXT_GROUP_SHAPES] + [(8, 128, 4, 56, 56, 1, 1), (8, 1024, 32, 14, 14, 2, 1)]
    sweep = _sweep(17)
    ran, one_by_one, names = 0, 0, set()
    for i, (n, c, cg, h, w, s, p) in enumerate(geo + sweep):
        if h + 2 * p < 3 or w + 2 * p < 3:      # (an empty output: not a convolution)
            continue
        in_dt, out_dt, relu = I8_COMBOS[i % len(I8_COMBOS)]
        conv, x, want, _ = _i8_case(rng, n, c, cg, h, w, s, p, in_dt, out_dt, relu, bias=bool((i // len(I8_COMBOS)) % 2))
        names |= set(_every_form(conv, x, want, ((n, c, cg, h, w, s, p), (in_dt, out_dt, relu))))
        ran += 1
        one_by_one += h == 1 and w == 1
    assert ran >= len(geo) + 40 and one_by_one >= 2, (ran, one_by_one)
    assert "direct_i8" in names and sum(a.startswith("g3x3_i8_") for a in names) >= 1, names
    print("grouped 3x3: %d geometries, kernels: %s" % (ran, " ".join(sorted(names))))


def _fixed_case(x, wq, ws, b, g, in_dt, out_dt, relu, pad, in_scale, out_scale):
    bp, sc = O.conv_i8_prepare(ws, b, in_scale, out_scale, in_dt, out_dt)
    want = O.conv_i8(x, wq, bp, sc, out_dt, relu, (pad, pad), (1, 1), group=g)
    n, h, w, c = x.shape
    prm = S.ConvParam(wq, b, g, (pad, pad), (1, 1), (1, 1), relu, ws)
    conv = S.SaberConv2D(True).init((n, c, h, w), prm, in_dt, out_dt, in_scale, out_scale, in_layout=L.NHWC, out_layout=L.NHWC)
    return conv, want


def test_group_isolation():
    """test 4a: C = 64, Cg = 4, every weight 127, u8 input 255 everywhere except ONE group's channels at 0: that group's outputs are the
    bias alone (the block-diagonal weight fragment multiplies its 12 foreign channels of the row block by zero), the others the oracle's"""
    c, cg, g = 64, 4, 16
    rng = np.random.default_rng(20272)
    wq = np.full((c, cg, 3, 3), 127, np.int8)
    ws = np.full(c, 0.01, np.float32)
    b = (rng.standard_normal(c) * 0.5 + 1.0).astype(np.float32)
    for quiet in (0, 5, 15):
        x = np.full((2, 6, 7, c), 255, np.uint8)
        x[..., quiet * cg:(quiet + 1) * cg] = 0
        conv, want = _fixed_case(x, wq, ws, b, g, L.U8, L.F32, False, 1, 0.02, 1.0)
        bp, sc = O.conv_i8_prepare(ws, b, 0.02, 1.0, L.U8, L.F32)
        alone = (bp * sc)[quiet * cg:(quiet + 1) * cg]
        assert np.array_equal(want[..., quiet * cg:(quiet + 1) * cg], np.broadcast_to(alone, want.shape[:3] + (cg,)))
        assert np.abs(want[..., :quiet * cg]).min(initial=1e9) > 40 and np.abs(want[..., (quiet + 1) * cg:]).min(initial=1e9) > 40
        _every_form(conv, torch.from_numpy(x).cuda(), want, ("isolation", quiet))


@pytest.mark.parametrize("c", [64, 128])
def test_padding_compensation_at_full_scale(c):
    """test 4b: Cg = 64, u8 input all 255, weights all -128 and then all 127, pad 1, on 3 x 3 and 5 x 4 images: corners (4 taps), edges (6)
    and the interior (9) equal the oracle; the interior accumulator exceeds 2^24 in magnitude. C = 64 is ONE group - an ordinary
    convolution on the implicit-GEMM kernels, compared all the same; C = 128 (two groups) is the smallest grouped conv with Cg = 64."""
    cg, g = 64, c // 64
    for wv in (-128, 127):
        for (h, w) in ((3, 3), (5, 4)):
            x = np.full((1, h, w, c), 255, np.uint8)
            wq = np.full((c, cg, 3, 3), wv, np.int8)
            ws = np.full(c, 1.0, np.float32)
            acc_in = 9 * cg * 255 * wv
            assert abs(acc_in) > 1 << 24
            for out_dt, out_scale in ((L.F32, 1.0), (L.S8, abs(acc_in) / 100.0)):
                conv, want = _fixed_case(x, wq, ws, None, g, L.U8, out_dt, False, 1, 1.0, out_scale)
                if out_dt == L.F32:      # (in_scale 1, w_scale 1: the f32 output is the rounded accumulator times 127 / 255)
                    k = np.float32(127.0) / np.float32(255.0)
                    assert want[0, 1, 1, 0] == np.float32(acc_in) * k and want[0, 0, 0, 0] == np.float32(4 * cg * 255 * wv) * k
                    assert want[0, 0, 1, 0] == np.float32(6 * cg * 255 * wv) * k
                xd = torch.from_numpy(x).cuda()
                if g == 1:
                    y = conv.new_output()
                    y.fill_(SENTINEL)
                    conv.dispatch(xd, y)
                    assert np.array_equal(_h(y), want), (wv, h, w, conv.algo())
                else:
                    _every_form(conv, xd, want, ("compensation", wv, h, w, out_dt))


@pytest.mark.parametrize("out_dt", [L.U8, L.S8])
def test_int8_saturation(out_dt):
    """test 5: out_scale = a quarter of the MAXABS scale - the oracle output holds both rails and unsaturated values, every form equals it"""
    rng = np.random.default_rng(20273 + out_dt)
    hi, lo = (255, 0) if out_dt == L.U8 else (127, -128)
    for (n, c, cg, h, w, s, p), in_dt in (((2, 128, 4, 14, 14, 1, 1), L.U8), ((1, 64, 32, 15, 9, 2, 1), L.S8), ((3, 256, 8, 7, 7, 1, 1), L.U8),
                                          ((1, 128, 64, 11, 20, 2, 0), L.S8), ((1, 192, 16, 9, 9, 1, 1), L.U8)):
        seed = int(rng.integers(1 << 30))
        _, _, _, scale = _i8_case(np.random.default_rng(seed), n, c, cg, h, w, s, p, in_dt, out_dt, False, True)
        # the same operands again (same generator state: same x, same weights) with a quarter of that scale
        conv, x, want, _ = _i8_case(np.random.default_rng(seed), n, c, cg, h, w, s, p, in_dt, out_dt, False, True, out_scale=scale / 4)
        assert np.count_nonzero(want == hi) > 0 and np.count_nonzero(want == lo) > 0, (out_dt, (n, c, cg, h, w, s, p))
        assert np.count_nonzero((want > lo) & (want < hi)) > 0
        _every_form(conv, x, want, ("saturation", (n, c, cg, h, w, s, p)))


@pytest.mark.parametrize("cg", [4, 8, 16, 32, 64])
def test_requantisation_ties(cg):
    """test 6: tests/int8_probe.py's depthwise recipe at Cg > 1 - one centre-tap weight per output channel: exact .5 ties of both parities
    and both signs, both rails and the op-order channels, s8 and u8 outputs from s8 and u8 inputs, relu on and off, stride 1 and 2"""
    c = 64 if cg < 64 else 128
    runs = 0
    for stride in (1, 2):
        geo = (1, 7, 9, c, c, 3, 1, stride)
        for idt, odt, relu in P.CONV_COMBOS:
            p, wq = GU.group_probe("group/cg%d/s%d" % (cg, stride), geo, cg, idt, odt, relu)
            P.assert_classes(p)
            bp, sc = O.conv_i8_prepare(p.w_scale, p.bias, p.in_scale, p.out_scale, idt, odt)
            assert np.array_equal(bp, p.bp) and np.array_equal(sc, p.sc)
            want = O.conv_i8(p.x, wq, bp, sc, odt, int(p.relu), (1, 1), (stride, stride), group=c // cg)
            assert np.array_equal(want, P.emulate(p)), p.name      # (the oracle agrees with the probe's own float32 model)
            prm = S.ConvParam(wq, p.bias, c // cg, (1, 1), (stride, stride), (1, 1), p.relu, p.w_scale)
            conv = S.SaberConv2D(True).init((1, c, 7, 9), prm, idt, odt, p.in_scale, p.out_scale, in_layout=L.NHWC, out_layout=L.NHWC)
            _every_form(conv, torch.from_numpy(p.x).cuda(), want, (p.name, idt, odt, relu))
            runs += 1
    assert runs == 16


@pytest.mark.parametrize("spelling", ["f32", "s8"])
def test_set_weights_twice_on_a_live_op(spelling):
    """test 7: saber_hip_conv2d_set_weights again on a live op, with one run in between: the second weights, bias and scales run in
    every form (the fragment planes and the compensation vector follow), the selection stays"""
    rng = np.random.default_rng(20274)
    lib = L.load()
    for (n, c, cg, h, s, p, in_dt) in ((2, 128, 8, 13, 1, 1, L.U8), (1, 64, 32, 9, 2, 1, L.U8), (1, 128, 64, 6, 1, 0, L.S8)):
        g = c // cg
        w1, w2 = [(rng.standard_normal((c, cg, 3, 3)) * 0.4).astype(np.float32) for _ in range(2)]
        b1, b2 = [(rng.standard_normal(c) * 0.5).astype(np.float32) for _ in range(2)]
        x = rng.integers(0, 256, (n, h, h, c)).astype(np.uint8) if in_dt == L.U8 else rng.integers(-128, 128, (n, h, h, c)).astype(np.int8)
        ws2 = O.weight_scales(w2)
        wq2 = O.quant_weights(w2, ws2)
        bp, sc = O.conv_i8_prepare(ws2, b2, 0.03, 0.9, in_dt, L.S8)
        want = O.conv_i8(x, wq2, bp, sc, L.S8, False, (p, p), (s, s), group=g)
        assert len(np.unique(want)) > 50
        xd = torch.from_numpy(x).cuda()
        conv = S.SaberConv2D(True).init((n, c, h, h), S.ConvParam(w1, b1, g, (p, p), (s, s), (1, 1), False), in_dt, L.S8, 0.02, 1.1,
                                        in_layout=L.NHWC, out_layout=L.NHWC)
        for label, code in _selections(conv)[1:]:
            conv.set_weights(w1, b1, None, 0.02, 1.1)
            conv.set_tile(code)
            y = conv.new_output()
            conv.dispatch(xd, y)
            first = _h(y).copy()
            if spelling == "f32":
                conv.set_weights(w2, b2, None, 0.03, 0.9)
            else:
                conv.set_weights(wq2, b2, ws2, 0.03, 0.9)
            assert lib.saber_hip_conv2d_get_tile(conv.h) == code
            y.fill_(SENTINEL)
            conv.dispatch(xd, y)
            got = _h(y)
            assert not np.array_equal(got, first)
            assert np.array_equal(got, want), ((n, c, cg, h, s, p), label, conv.algo())


# ---- ResNeXt-50 through the executor --------------------------------------------------------------------------------------------------
def _group_ops(net):
    return [i for i, c in enumerate(net.choices()) if (c >> 16) & 0xff == V]


def _force(net, v):
    ch = net.choices()
    idx = [i for i, c in enumerate(ch) if (c >> 16) & 0xff == V]
    assert len(idx) == 16, idx
    for i in idx:
        ch[i] = (V << 16) | v
    net.set_choices(ch)
    return idx


@pytest.fixture(scope="module")
def resnext():
    L.require_device()
    model = W.build_model("resnext50_32x4d")
    fw = W.framework_model(model, "int8")
    cache = {}

    def at(batch, hw):
        if (batch, hw) not in cache:
            x = W.make_input(batch, hw=hw)
            scales = W.calibrate(model, x)
            cache[(batch, hw)] = (x, scales, DU.run_int8(fw, scales, x))
        return cache[(batch, hw)]
    return model, fw, at


def _check_int8_net(net, x, ref, what, at_least):
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
        assert checked >= at_least and not net.unwritten("fc1000"), (what, checked)
        return checked
    xd = torch.from_numpy(x).cuda()
    net.tensor("data").copy_(xd)
    net.run()
    n = compare()
    net.tensor("fc1000").zero_()
    net.capture()
    net.replay()
    compare()
    net.autotune(iters=2)
    net.tensor("data").copy_(xd)
    net.run()
    compare()
    return n


@pytest.mark.parametrize("fuse", [False, True])
@pytest.mark.parametrize("batch,hw", [(3, 64), (1, 224), (8, 224)])
def test_resnext50_int8_every_edge_bit_exact(resnext, batch, hw, fuse):
    """test 8: ResNeXt-50 INT8 (the framework's op list) unfused and with the default fusions - which were written for ResNet's
    C -> 4C -> C blocks and must decline or keep the bits on C -> 2C -> C; eager, replayed, autotuned; with the static selection and with
    every form (the direct kernel included) forced on the 16 grouped ops"""
    model, fw, at = resnext
    x, scales, ref = at(batch, hw)
    probe = W.build_int8_net(fw, dict(scales), batch, hw=hw, fuse=fuse)
    gi = _group_ops(probe)
    assert len(gi) == 16
    forms = GU.group_forms(L.load(), next(k for k in probe.keep if getattr(getattr(k, "desc", None), "group", 1) > 1).h)
    assert len(forms) >= 1
    # unfused: 53 convs, pool1, 16 sums, pool5, the fc and prob are all written; fused: at least the grouped convs' inputs or outputs
    at_least = 73 if not fuse else 20
    for v in [None, 0] + forms:
        net = probe if v is None else W.build_int8_net(fw, dict(scales), batch, hw=hw, fuse=fuse)
        if v is not None:
            idx = _force(net, v)
            names = [net.op_name(i) for i in idx]
            assert sum(1 for nm in names if ("g3x3_i8_" in nm if v else "direct_i8" in nm)) == 16, names
        n = _check_int8_net(net, x, ref, (batch, hw, fuse, v), at_least)
    print("ResNeXt-50 INT8 batch %d hw %d fuse %s: %d edges compared, forms %s" % (batch, hw, fuse, n, forms))


@pytest.mark.parametrize("fuse", [False, True])
def test_resnext50_int8_batch_invariance(resnext, fuse):
    """test 8, last item: with ONE set of scales, image 0 of the batch of 8 equals the same image alone, on the device and in the oracle"""
    model, fw, at = resnext
    x8, s8, ref8 = at(8, 224)
    n8 = W.build_int8_net(fw, dict(s8), 8, fuse=fuse)
    n1 = W.build_int8_net(fw, dict(s8), 1, fuse=fuse)
    n8.tensor("data").copy_(torch.from_numpy(x8).cuda())
    n1.tensor("data").copy_(torch.from_numpy(x8[:1]).cuda())
    n8.run()
    n1.run()
    assert np.array_equal(_h(n8.tensor("fc1000"))[0], _h(n1.tensor("fc1000"))[0])
    assert np.array_equal(_h(n1.tensor("fc1000"))[0], ref8["fc1000"][0])


def test_resnext50_fp32_every_edge():
    """test 9: ResNeXt-50 FP32 at 64 x 64, batch 2: every produced edge within the project's two 1e-4 criteria of the oracle walk. The
    grouped layers run on the direct FP32 kernel: the model entry works in both precisions."""
    L.require_device()
    model = W.build_model("resnext50_32x4d")
    x = W.make_input(2, hw=64)
    ref = DU.run_fp32(model, x)
    net = W.build_fp32_net(model, 2, hw=64)
    names = [net.op_name(i) for i in range(net.num_ops())]
    assert sum("direct_f32" in nm for nm in names) == 16, names
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
        assert e_max <= FP32_RTOL and e_el <= FP32_RTOL, (name, e_max, e_el)
        checked += 1
    assert done == net.num_ops() - 1 and checked >= 50, checked
