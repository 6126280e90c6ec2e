"""Concat and SqueezeNet v1.1 on the GPU: the channel-concat kernel (elementwise.hip: concat_nhwc_kernel; saber_hip_concat_nhwc) between
guard bands against tests/fire_util.py's restatement of the reference's arithmetic, the concat op inside the executor (every input seen
by the lanes, the arena planner, capture / replay and the op-list capture), and squeezenet_v1_1 end to end through the default executor:
INT8 every written edge bit for bit against the oracle walk, FP32 within 1e-4 on every edge."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from anakin_amd import lib as L  # noqa: E402
from anakin_amd import saber as S  # noqa: E402
from anakin_amd import workloads as W  # noqa: E402
from tests import fire_util as FU  # noqa: E402
from tests import guard_util as GU  # noqa: E402

POISON = 77


@pytest.fixture(scope="module", autouse=True)
def _device():
    L.require_device()  # fail loudly: no fallback path exists


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


# ---- the kernel between guard bands ------------------------------------------------------------------------------------------------------
def concat_guarded(name, mult):
    dt, pixels, chans = FU.CONCAT_CASES[name]
    xs = FU.concat_inputs(name)
    want = FU.concat_ref(xs, mult)
    n = len(xs)
    ch = (C.c_int * n)(*chans)
    m = None if mult is None else (C.c_float * n)(*mult)

    def launch(T, ws):
        ptrs = (C.c_void_p * n)(*[T["x%d" % i].data_ptr() for i in range(n)])
        L.check(L.load().saber_hip_concat_nhwc(pixels, n, ptrs, ch, m, dt, T["y"].data_ptr(), torch.cuda.current_stream().cuda_stream))

    def plain(inputs, outputs, ws_bytes):
        T = {k: dev(v) for k, v in inputs.items()}
        T["y"] = torch.full(want.shape, POISON, dtype=GU.torch_dtype(want.dtype), device="cuda") if want.dtype != np.float32 else \
            torch.full(want.shape, float("nan"), device="cuda")
        return T, None
    got = GU.run_guarded({"x%d" % i: x for i, x in enumerate(xs)}, {"y": (want.shape, want.dtype, None)}, launch, plain=plain,
                         what="concat %s%s" % (name, "" if mult is None else " x %s" % (mult,)))["y"]
    assert GU.same_bytes(got, want), (name, mult, int(np.count_nonzero(got != want)), want.size)


@pytest.mark.parametrize("name", sorted(FU.CONCAT_CASES))
def test_concat_is_a_copy_between_guard_bands(name):
    """f32 / s8 / u8, 1 / 2 / 3 / 8 inputs, channel counts 1, 3, 16, 48, 100: 16-byte, 4-byte and 1-byte lanes, offsets that break the
    alignment of an otherwise aligned input; payloads are 16-byte aligned and no more, nothing outside any tensor is written or used"""
    concat_guarded(name, None)


@pytest.mark.parametrize("name", sorted(FU.CONCAT_MULTS))
def test_u8_concat_rescales_with_round_to_even_and_saturation(name):
    """multipliers 1, < 1 and > 1: the u8 branch of the reference (float32 product, round to nearest even, unsigned saturation)"""
    mult = FU.CONCAT_MULTS[name]
    xs = FU.concat_inputs(name)
    want = FU.concat_ref(xs, mult)
    off = 0
    for x, m in zip(xs, mult):      # the cases do what they are there for: ties that round down, the rail
        if m in (0.5, 1.5, 2.5):
            _, tie = FU.concat_u8_f64(x, m)
            assert tie.any()
        if m >= 1.5:
            assert np.count_nonzero(want[:, off:off + x.shape[1]] == 255) > np.count_nonzero(x == 255)
        off += x.shape[1]
    concat_guarded(name, mult)


def test_saber_concat_wrapper_takes_scales_the_references_way():
    """S.SaberConcat: out scale = the largest input scale, m_i = scale_max / scale_i; NHWC tensors in, NHWC out"""
    rng = np.random.default_rng(5)
    xs = [rng.integers(0, 256, (2, 5, 7, c)).astype(np.uint8) for c in (16, 48, 3)]
    scales = [0.031, 0.05, 0.0125]
    cat = S.SaberConcat().init([16, 48, 3], L.U8, scales)
    mult, out_scale = FU.concat_multipliers(scales)
    assert cat.out_scale == out_scale and np.array_equal(cat.mult, mult) and mult[1] == 1.0
    got = host(cat.dispatch([dev(x) for x in xs]))
    assert got.shape == (2, 5, 7, 67) and np.array_equal(got, FU.concat_ref(xs, mult))
    xf = [rng.standard_normal((3, 4, 4, c)).astype(np.float32) for c in (8, 24)]
    got = host(S.SaberConcat().init([8, 24], L.F32).dispatch([dev(x) for x in xf]))
    assert GU.same_bytes(got, np.concatenate(xf, -1))


# ---- the op inside the executor -------------------------------------------------------------------------------------------------------------
def _branchy_net(lanes, compact=False):
    """x -> three eltwise ops (a, b, c) -> concat3 -> two more eltwise ops -> out, out2. With `lanes` b and c run on the side stream: the
    concat's THIRD input is then produced on the other lane, which only a lane logic that sees every input orders. For the arena
    planner: `out` is as large as a + b + c and lives after them, so a plan that took c for dead after its producer would lay c
    under `cat`."""
    n, h, w, c = 2, 13, 13, 48
    rng = np.random.default_rng(11)
    x = rng.integers(-128, 128, (n, h, w, c)).astype(np.int8)
    net = S.Net()
    net.add_tensor("x", (n, h, w, c), L.S8)
    for nm in ("a", "b", "c"):
        net.add_tensor(nm, (n, h, w, c), L.S8)
    net.add_tensor("cat", (n, h, w, 3 * c), L.S8)
    net.add_tensor("out", (n, h, w, 3 * c), L.S8)
    net.add_tensor("out2", (n, h, w, 3 * c), L.S8)
    cnt = n * h * w * c
    coeffs = {"a": 0.5, "b": 0.25, "c": 0.75}
    for nm in ("a", "b", "c"):
        net.add_eltwise_i8(cnt, 1.0, 1.0, coeffs[nm], coeffs[nm], False, "x", "x", nm)
    net.add_concat(["a", "b", "c"], "cat")
    net.add_eltwise_i8(3 * cnt, 1.0, 1.0, 0.5, 0.5, True, "cat", "cat", "out")
    net.add_eltwise_i8(3 * cnt, 1.0, 1.0, 1.0, 0.5, False, "out", "out", "out2")
    assert [net.op_name(i) for i in range(net.num_ops())][3] == "concat3"
    if lanes:
        net.set_lane(1, 1)
        net.set_lane(2, 1)
    net.finalize()
    from oracle import oracle as O
    ref = {nm: O.eltwise_i8(x, x, 1.0, 1.0, np.float32(v), np.float32(v), False) for nm, v in coeffs.items()}
    ref["cat"] = np.concatenate([ref["a"], ref["b"], ref["c"]], -1)
    ref["out"] = O.eltwise_i8(ref["cat"], ref["cat"], 1.0, 1.0, np.float32(0.5), np.float32(0.5), True)
    ref["out2"] = O.eltwise_i8(ref["out"], ref["out"], 1.0, 1.0, np.float32(1.0), np.float32(0.5), False)
    return net, x, ref


@pytest.mark.parametrize("lanes", [False, True])
def test_concat_op_eager_replayed_and_across_lanes(lanes):
    net, x, ref = _branchy_net(lanes)
    work = net.op_work(3)
    assert work == (2.0 * ref["cat"].size, 0.0)      # bytes read + written, no flops
    for mode in ("eager", "replayed"):
        for nm in ("a", "b", "c", "cat", "out", "out2"):
            net.tensor(nm).fill_(POISON)
        net.tensor("x").copy_(dev(x))
        if mode == "eager":
            net.run()
        else:
            net.capture()
            net.replay()
        for nm in ("a", "b", "c", "cat", "out", "out2"):
            assert np.array_equal(host(net.tensor(nm)), ref[nm]), (lanes, mode, nm)


def test_arena_planner_keeps_every_concat_input_alive():
    """after compact_arena the three inputs of the concat - the third as much as the first two - still hold their values when it runs"""
    net, x, ref = _branchy_net(False)
    before = net.arena_bytes()
    net.compact()
    assert net.compacted() and net.arena_bytes() < before
    net.tensor("x").copy_(dev(x))
    net.run()
    assert np.array_equal(host(net.tensor("out2")), ref["out2"])


@pytest.mark.parametrize("slot", [0, 1, 2])
def test_optimizer_counts_a_concat_input_in_any_position_as_a_consumer(slot):
    """conv -> t (s8), eltwise(t, r) -> e, and a concat3 that ALSO reads t in position `slot`. Flag 1 fuses conv + eltwise only where the
    eltwise is t's single consumer - it then removes the edge t. A concat that reads t, as its third input as much as its first,
    is a consumer: nothing is fused, t stays written, the concat holds the conv's bytes. Without the concat the same list IS fused."""
    from oracle import oracle as O
    n, h, w, c, k = 1, 6, 7, 64, 64      # (an implicit-GEMM conv: the shape class flag 1 fuses in the ResNets)
    rng = np.random.default_rng(20 + slot)
    x = rng.integers(0, 256, (n, h, w, c)).astype(np.uint8)
    r = rng.integers(-128, 128, (n, h, w, k)).astype(np.int8)
    p, q = (rng.integers(-128, 128, (n, h, w, k)).astype(np.int8) for _ in range(2))
    wt = (rng.standard_normal((k, c, 1, 1)) * 0.25).astype(np.float32)
    bias = rng.standard_normal(k).astype(np.float32) * 0.3
    s_in, s_t, s_r, s_e = 0.02, 0.04, 0.05, 0.07
    ws = O.weight_scales(wt)
    bp, sc = O.conv_i8_prepare(ws, bias, s_in, s_t, O.U8, O.S8)
    t_ref = O.conv_i8(x, O.quant_weights(wt, ws), bp, sc, O.S8, 0, (0, 0), (1, 1))
    coeff = np.float32(1.0 / s_e)
    e_ref = O.eltwise_i8(t_ref, r, s_t, s_r, coeff, coeff, True)

    def build(with_concat):
        net = S.Net()
        for nm, ch, dt in (("x", c, L.U8), ("t", k, L.S8), ("r", k, L.S8), ("e", k, L.S8), ("p", k, L.S8), ("q", k, L.S8), ("cat", 3 * k, L.S8)):
            net.add_tensor(nm, (n, h, w, ch), dt)
        conv = S.SaberConv2D(True).init((n, c, h, w), S.ConvParam(wt, bias, 1, (0, 0), (1, 1), (1, 1), False), L.U8, L.S8, s_in, s_t,
                                        in_layout=L.NHWC, out_layout=L.NHWC)
        net.add_conv(conv, "x", "t")
        net.add_eltwise_i8(n * h * w * k, s_t, s_r, float(coeff), float(coeff), True, "t", "r", "e")
        srcs = ["p", "q"]
        srcs.insert(slot, "t")
        if with_concat:
            net.add_concat(srcs, "cat")
        removed = net.optimize(15)
        net.finalize()
        for nm, a in (("x", x), ("r", r), ("p", p), ("q", q)):
            net.tensor(nm).copy_(dev(a))
        for nm in ("e", "cat"):
            net.tensor(nm).fill_(POISON)
        net.run()
        return net, removed, srcs
    net, removed, srcs = build(True)
    assert removed == 0 and net.num_ops() == 3 and not net.unwritten("t"), (slot, removed)
    assert np.array_equal(host(net.tensor("t")), t_ref) and np.array_equal(host(net.tensor("e")), e_ref)
    want = np.concatenate([{"t": t_ref, "p": p, "q": q}[nm] for nm in srcs], -1)
    assert np.array_equal(host(net.tensor("cat")), want), slot
    net, removed, _ = build(False)      # the control: with the eltwise as the only reader the conv takes it as its epilogue
    assert removed == 1 and net.num_ops() == 1 and net.unwritten("t")
    assert np.array_equal(host(net.tensor("e")), e_ref)


def test_resnet50_int8_op_names_and_choices_are_the_parent_commits():
    """ResNet50 INT8 built as bench.py builds it (batch 1 and 8): op names, static choices and launch count equal what the commit
    before the concat operator gave (recorded from that commit's library on an MI355X: tests/golden/resnet50_int8_ops_parent.json) -
    the optimiser's and the lanes' view of an op's inputs changed for concat ops only"""
    import json
    import os
    want = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "resnet50_int8_ops_parent.json")))
    model = W.build_model("resnet50")
    fw = W.framework_model(model, "int8")
    for batch in (1, 8):
        x = W.make_input(batch)
        net = W.build_int8_net(fw, dict(W.calibrate(model, x)), batch)
        rec = want["b%d" % batch]
        assert [net.op_name(i) for i in range(net.num_ops())] == rec["names"], batch
        assert net.choices() == rec["choices"] and net.num_launches() == rec["launches"], batch


def test_concat_is_recorded_by_the_op_list_capture():
    rng = np.random.default_rng(3)
    xs = [rng.integers(0, 256, (30, c)).astype(np.uint8) for c in (16, 3, 100)]
    mult = [1.5, 1.0, 0.5]
    cat = S.SaberConcat().init([16, 3, 100], L.U8, None)
    cat.mult = np.asarray(mult, np.float32)
    d = [dev(v) for v in xs]
    y = torch.full((30, 119), POISON, dtype=torch.uint8, device="cuda")
    with S.Capture() as cap:
        cat.dispatch(d, out=y)
    assert host(y).min() == POISON == host(y).max()      # recorded, not launched
    net = cap.net
    assert net.num_ops() == 1 and net.op_name(0) == "concat3"
    net.bind(net.tensor_of_ptr(y), y)
    net.finalize()
    net.run()
    assert np.array_equal(host(y), FU.concat_ref(xs, mult))


# ---- SqueezeNet v1.1 through the executor ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def squeezenet():
    model = W.build_model("squeezenet_v1_1")
    fw = W.framework_model(model, "int8")
    cache = {}

    def at(batch, hw):
        if (batch, hw) not in cache:
            x = W.make_input(batch, hw=hw)
            scales = W.calibrate(model, x)
            cache[(batch, hw)] = (x, scales, FU.run_int8(fw, scales, x))
        return cache[(batch, hw)]
    return model, fw, at


def compare_int8(net, ref, what, at_least):
    torch.cuda.synchronize()
    checked = 0
    for name in net.tensors:
        if name == "data" or net.unwritten(name):
            continue
        got, want = host(net.tensor(name)), ref[name]
        if want.dtype == np.float32:      # pool10 (f32 average of a dequantised edge) and prob
            assert np.abs(got.reshape(want.shape) - want).max() <= 1e-4 * np.abs(want).max(), (what, name)
        else:
            assert got.dtype == want.dtype and np.array_equal(got, want.reshape(got.shape)), (what, name, int(np.count_nonzero(got != want.reshape(got.shape))))
        checked += 1
    assert checked >= at_least, (what, checked)


def run_passes(net, x, ref, what, at_least):
    for name in net.tensors:
        if name != "data" and not net.unwritten(name):
            net.tensor(name).fill_(POISON) if net.tensors[name][2] != torch.float32 else net.tensor(name).fill_(float("nan"))
    net.tensor("data").copy_(torch.from_numpy(x).cuda())
    net.run()
    compare_int8(net, ref, (what, "eager"), at_least)
    net.tensor("prob").zero_()
    net.tensor("fire9_concat").fill_(POISON)
    net.capture()
    net.replay()
    compare_int8(net, ref, (what, "replayed"), at_least)


@pytest.mark.parametrize("batch,hw", [(1, 224), (2, 63), (1, 63)])
def test_squeezenet_int8(squeezenet, batch, hw):
    """the framework op list one launch per operator, and through the default executor flags: every written edge bit for bit"""
    model, fw, at = squeezenet
    x, scales, ref = at(batch, hw)
    net = W.build_int8_net(fw, dict(scales), batch, hw=hw, fuse=False)
    assert net.num_ops() == net.num_launches() == 26 + 3 + 8 + 2      # convs, max poolings, concats, pool10 + prob
    names = [net.op_name(i) for i in range(net.num_ops())]
    assert names.count("concat2") == 8
    run_passes(net, x, ref, (batch, hw, "unfused"), 39)
    net = W.build_int8_net(fw, dict(scales), batch, hw=hw)
    assert [net.op_name(i) for i in range(net.num_ops())].count("concat2") == 8
    run_passes(net, x, ref, (batch, hw, "default"), 38)
    if (batch, hw) == (2, 63):      # the autotuned selection and a compacted arena compute the same classes
        net.autotune(iters=2)
        run_passes(net, x, ref, (batch, hw, "autotuned"), 38)
        net.compact()
        net.tensor("data").copy_(torch.from_numpy(x).cuda())
        net.run()
        got = host(net.tensor("prob"))
        assert np.abs(got - ref["prob"]).max() <= 1e-4 * ref["prob"].max()


def test_squeezenet_int8_with_unequal_concat_input_scales(squeezenet):
    """scales that calibrate() did not equalise: the concat takes the larger one and rescales the other input (multipliers != 1 through
    W.build_int8_net -> S.SaberConcat -> saber_hip_net_add_concat), still bit for bit the oracle walk on every edge"""
    model, fw, at = squeezenet
    x, scales, _ = at(1, 63)
    scales = dict(scales)
    scales["fire4_expand1x1"] *= 0.75      # m = 1 / 0.75 for the first input of fire4_concat
    scales["fire7_expand3x3"] *= 0.5       # m = 2 for the second input of fire7_concat: ties and the rail
    ref = FU.run_int8(fw, scales, x)
    mult, _ = FU.concat_multipliers([scales["fire7_expand1x1"], scales["fire7_expand3x3"]])
    assert mult[0] == 1.0 and mult[1] == 2.0
    assert not np.array_equal(ref["fire7_concat"][..., 192:], ref["fire7_expand3x3"]) and np.array_equal(ref["fire7_concat"][..., :192], ref["fire7_expand1x1"])
    net = W.build_int8_net(fw, dict(scales), 1, hw=63)
    run_passes(net, x, ref, "unequal scales", 38)


@pytest.mark.parametrize("batch,hw", [(1, 224), (2, 63)])
def test_squeezenet_fp32(squeezenet, batch, hw):
    """FP32: every edge within 1e-4 of the oracle's naive forward, relative to the edge's largest magnitude"""
    model, fw, at = squeezenet
    x = W.make_input(batch, hw=hw)
    ref = FU.run_fp32(model, x)
    net = W.build_fp32_net(model, batch, hw=hw)
    assert [net.op_name(i) for i in range(net.num_ops())].count("concat2") == 8
    net.tensor("data").copy_(torch.from_numpy(x).cuda())
    net.run()
    checked = 0
    for name in net.tensors:
        if name in ("data", "data_nhwc") or name not in ref:
            continue
        got, want = host(net.tensor(name)), ref[name]
        if got.ndim == 4:
            got = got.transpose(0, 3, 1, 2)      # NHWC on the device, NCHW in the oracle
        err = float(np.abs(got.reshape(want.shape) - want).max() / max(np.abs(want).max(), 1e-30))
        assert err <= 1e-4, (batch, hw, name, err)
        checked += 1
    assert checked >= 36, checked      # (conv1 runs inside a fused conv + pooling launch where the library has one)
