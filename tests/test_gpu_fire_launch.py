"""The Fire module as one INT8 launch on the GPU (conv_fire.hip: fire_squeeze_expand_i8; saber_hip_conv2d_fire_*): every accepted form of
every geometry and variant of tests/fire_util.py equals the oracle - O.conv_i8 (squeeze) -> O.conv_i8 x 2 -> np.concatenate - bit for bit on
y and, when requested, on y_squeeze, and equals the library's own four launches; through the executor (saber_hip_net_optimize flag 65536)
the flag off, the static choice, each form forced and the autotuned selection give identical bytes on every written edge."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from anakin_amd import lib as L  # noqa: E402
from anakin_amd import saber as S  # noqa: E402
from tests import fire_util as FU  # noqa: E402
from tests import guard_util as GU  # noqa: E402

POISON = 77
NHWC = dict(in_layout=L.NHWC, out_layout=L.NHWC)


@pytest.fixture(scope="module", autouse=True)
def _device():
    L.require_device()  # fail loudly: no fallback path exists


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def module_of(cs):
    c, s, e1, e3, h, w, n = cs.geo
    sq = S.SaberConv2D(True).init((n, c, h, w), S.ConvParam(cs.w_s, cs.b_s, 1, (0, 0), (1, 1), (1, 1), True), cs.idt, L.U8, FU.IN_SCALE, cs.s_scale, **NHWC)
    a = S.SaberConv2D(True).init((n, s, h, w), S.ConvParam(cs.w_1, cs.b_1, 1, (0, 0), (1, 1), (1, 1), True), L.U8, L.U8, cs.s_scale, cs.e1_scale, **NHWC)
    b = S.SaberConv2D(True).init((n, s, h, w), S.ConvParam(cs.w_3, cs.b_3, 1, (1, 1), (1, 1), (1, 1), True), L.U8, L.U8, cs.s_scale, cs.e3_scale, **NHWC)
    return sq, a, b


def forms_of(fire):
    keep = fire.tile()
    lib = L.load()
    codes = [c for c in range(1, FU.FIRE_MAX_CODE + 1) if lib.saber_hip_conv2d_fire_set_tile(fire.h, c) == 0]
    fire.set_tile(keep)
    return codes


def run_case(cs, min_forms=2):
    """outputs poisoned before each run; the four separate launches and every form equal the oracle bit for bit on y and y_squeeze; y is
    identical with y_squeeze NULL, which is then not written"""
    what = (cs.geo, cs.idt, cs.bias)
    c, s, e1, e3, h, w, n = cs.geo
    sq, a, b = module_of(cs)
    xd = dev(cs.x)
    y_s, y_a, y_b = sq.new_output(), a.new_output(), b.new_output()
    for t in (y_s, y_a, y_b):
        t.fill_(POISON)
    sq.dispatch(xd, y_s)
    a.dispatch(y_s, y_a)
    b.dispatch(y_s, y_b)
    y4 = host(S.SaberConcat().init([e1, e3], L.U8).dispatch([y_a, y_b]))
    assert np.array_equal(host(y_s), cs.s), (what, "separate launches, squeeze", sq.algo())
    assert np.array_equal(host(y_a), cs.e1) and np.array_equal(host(y_b), cs.e3), (what, "separate launches, expands", a.algo(), b.algo())
    assert np.array_equal(y4, cs.y), (what, "four launches")
    fire = S.SaberConvFire(sq, a, b)
    codes = forms_of(fire)
    assert len(codes) >= min_forms, (what, codes)
    y = torch.empty((n, h, w, e1 + e3), dtype=torch.uint8, device="cuda")
    for code in codes:
        fire.set_tile(code)
        assert fire.tile() == code and fire.algo().startswith("fire_squeeze_expand_i8_"), (what, code, fire.algo())
        y.fill_(POISON)
        y_s.fill_(POISON)
        fire.dispatch(xd, y, y_s)
        got = host(y)
        assert np.array_equal(got, cs.y), (what, fire.algo(), "y vs oracle", int(np.count_nonzero(got != cs.y)), cs.y.size,
                                           int(np.count_nonzero(got[..., :e1] != cs.e1)), int(np.count_nonzero(got[..., e1:] != cs.e3)))
        assert np.array_equal(got, y4), (what, fire.algo(), "y vs the four launches")
        assert np.array_equal(host(y_s), cs.s), (what, fire.algo(), "y_squeeze")
        y.fill_(POISON)
        y_s.fill_(POISON)
        fire.dispatch(xd, y)
        assert np.array_equal(host(y), cs.y), (what, fire.algo(), "y without y_squeeze")
        assert int(host(y_s).min()) == POISON == int(host(y_s).max()), (what, fire.algo(), "NULL y_squeeze was written")
    return codes


@pytest.mark.parametrize("name", sorted(FU.GEOMETRIES))
def test_geometries_every_form_bit_exact(name):
    assert run_case(FU.fire_case(name)) == [1, 2]


@pytest.mark.parametrize("name", ["a", "c", "f", "g2"])
def test_s8_input(name):
    run_case(FU.fire_case(name, idt=FU.S8))


@pytest.mark.parametrize("bi", range(len(FU.BIASES)))
def test_every_bias_pattern(bi):
    run_case(FU.fire_case("f", bi=bi))
    run_case(FU.fire_case("b", idt=FU.S8, bi=bi))


def test_distinct_expand_scales():
    for name in ("c", "f"):
        cs = FU.fire_case(name)
        assert cs.e1_scale != cs.e3_scale
        run_case(cs)


@pytest.mark.parametrize("name", ["c", "f"])
def test_saturation(name):
    cs = FU.fire_case(name, sat=True)
    for half in (cs.s, cs.e1, cs.e3):      # saturated and unsaturated bytes on the squeeze edge and on each half
        hi, mid = FU.saturation(half)
        assert hi > 10 and mid > 10
    run_case(cs)


@pytest.mark.parametrize("name", ["a", "b", "g1", "g2"])
def test_zero_padding_of_the_squeeze_edge(name):
    """all-zero input, positive squeeze biases: a kernel that computed its halo pixels outside the image would store e3_with_computed_halo"""
    cs = FU.fire_case(name, zero_x=True)
    assert not np.array_equal(cs.e3_with_computed_halo(), cs.e3)
    run_case(cs)


@pytest.mark.parametrize("name", ["a", "d", "f"])
def test_guard_bands(name):
    """every form between guard bands, 16-byte-aligned-and-no-more payloads: nothing outside x, y or y_squeeze is written or used"""
    cs = FU.fire_case(name)
    c, s, e1, e3, h, w, n = cs.geo
    fire = S.SaberConvFire(*module_of(cs))
    for code in forms_of(fire):
        fire.set_tile(code)

        def launch(T, ws):
            fire.dispatch(T["x"], T["y"], T["y_s"])
        got = GU.run_guarded({"x": cs.x}, {"y": (cs.y.shape, np.uint8, None), "y_s": (cs.s.shape, np.uint8, None)}, launch, what="fire %s form %d" % (name, code))
        assert np.array_equal(got["y"], cs.y) and np.array_equal(got["y_s"], cs.s), (name, code)


def test_set_tile_and_create_refusals():
    cs = FU.fire_case("a")
    sq, a, b = module_of(cs)
    fire = S.SaberConvFire(sq, a, b)
    lib = L.load()
    keep, name = fire.tile(), fire.algo()
    for bad in (0, 3, -1, 99):
        assert lib.saber_hip_conv2d_fire_set_tile(fire.h, bad) == -2
        assert fire.tile() == keep and fire.algo() == name
    with pytest.raises(L.SaberHipError) as e:      # the expand convs swapped: the first is not a 1x1
        S.SaberConvFire(sq, b, a)
    assert e.value.status == L.UNIMPL


# ---- through the executor: saber_hip_net_optimize flag 65536 --------------------------------------------------------------------------------
FIRE_FLAG = 65536


def fire_sites(net):
    """[(op index, form code now selected)] of the squeeze ops that record a Fire decision (bit 31 without bit 30 of their choice)"""
    return [(i, (c >> 24) & 15) for i, c in enumerate(net.choices()) if (c >> 30) & 3 == 2]


def force(net, code):
    lib = L.load()
    for i, _ in fire_sites(net):
        base = net.choices()[i] & ~(15 << 24)
        assert lib.saber_hip_net_set_choice(net.h, i, base | (code << 24)) == 0, (i, code)
    return fire_sites(net)


class MiniNet:
    """two Fire modules behind each other at 13 x 13 (the second reads the first one's concat), with the oracle's edges"""

    def __init__(self, flag):
        m1, m2 = FU.fire_case("c"), None
        c, s, e1, e3, h, w, n = m1.geo
        # the second module's input is the first one's output: same geometry class, C = E1 + E3
        rng = np.random.default_rng(77)
        geo2 = (e1 + e3, 48, 64, 80, h, w, n)
        m2 = FU.FireCase(geo2, FU.U8, (True, True, True), 4242)
        m2.x = m1.y      # replace its random input by the real edge and walk it again
        m2 = _rewalk(m2, max(m1.e1_scale, m1.e3_scale))
        self.m1, self.m2 = m1, m2
        net = S.Net()
        net.add_tensor("x", (n, h, w, c), L.U8)
        self.ref = {}
        src, src_scale = "x", FU.IN_SCALE
        for tag, m, cat_scales in (("f1", m1, None), ("f2", m2, None)):
            cc, ss, a1, a3 = m.geo[:4]
            ops = [S.SaberConv2D(True).init((n, cc, h, w), S.ConvParam(m.w_s, m.b_s, 1, (0, 0), (1, 1), (1, 1), True), L.U8, L.U8, src_scale, m.s_scale, **NHWC),
                   S.SaberConv2D(True).init((n, ss, h, w), S.ConvParam(m.w_1, m.b_1, 1, (0, 0), (1, 1), (1, 1), True), L.U8, L.U8, m.s_scale, m.e1_scale, **NHWC),
                   S.SaberConv2D(True).init((n, ss, h, w), S.ConvParam(m.w_3, m.b_3, 1, (1, 1), (1, 1), (1, 1), True), L.U8, L.U8, m.s_scale, m.e3_scale, **NHWC)]
            for nm, ch in ((tag + "_s", ss), (tag + "_a", a1), (tag + "_b", a3), (tag + "_y", a1 + a3)):
                net.add_tensor(nm, (n, h, w, ch), L.U8)
            net.add_conv(ops[0], src, tag + "_s")
            net.add_conv(ops[1], tag + "_s", tag + "_a")
            net.add_conv(ops[2], tag + "_s", tag + "_b")
            net.add_concat([tag + "_a", tag + "_b"], tag + "_y")      # (multipliers 1: the bytes of the two convs)
            self.ref.update({tag + "_s": m.s, tag + "_a": m.e1, tag + "_b": m.e3, tag + "_y": m.y})
            src, src_scale = tag + "_y", max(m.e1_scale, m.e3_scale)
        assert net.optimize(15) == 0
        self.sites = net.optimize(FIRE_FLAG) if flag else 0
        net.finalize()
        self.net, self.x = net, m1.x


def _rewalk(m, in_scale):
    """the oracle edges of module m for the input m.x at scale in_scale (FireCase's stage, scales kept)"""
    from oracle import oracle as O

    def conv(src, src_scale, wt, b, out_scale, pad=0):
        ws = O.weight_scales(wt)
        bp, sc = O.conv_i8_prepare(ws, b, src_scale, out_scale, O.U8, O.U8)
        return O.conv_i8(src, O.quant_weights(wt, ws), bp, sc, O.U8, 1, (pad, pad), (1, 1))
    m.s = conv(m.x, in_scale, m.w_s, m.b_s, m.s_scale)
    m.e1 = conv(m.s, m.s_scale, m.w_1, m.b_1, m.e1_scale)
    m.e3 = conv(m.s, m.s_scale, m.w_3, m.b_3, m.e3_scale, 1)
    m.y = np.concatenate([m.e1, m.e3], -1)
    return m


def check_mini(mn, what, n_on):
    net = mn.net
    inner = [t + e for t in ("f1", "f2") for e in ("_s", "_a", "_b")]
    names = [net.op_name(i) for i in range(net.num_ops())]
    assert net.num_ops() == 8 and net.num_launches() == 8 - 3 * n_on, (what, names)
    assert sum(1 for nm in inner if net.unwritten(nm)) == 3 * n_on, (what, [nm for nm in inner if net.unwritten(nm)])
    for i, f in fire_sites(net):
        assert ("fire_squeeze_expand_i8_" in names[i]) == bool(f), (what, names)
        assert [names[i + 1], names[i + 2], names[i + 3]] == (["conv:(in the fire launch)"] * 2 + ["concat2 (in the fire launch)"] if f else names[i + 1:i + 3] + ["concat2"]), (what, names)
    out = {}
    for mode in ("eager", "replayed"):
        for nm in mn.ref:
            if not net.unwritten(nm):
                net.tensor(nm).fill_(POISON)
        net.tensor("x").copy_(dev(mn.x))
        if mode == "eager":
            net.run()
        else:
            net.capture()
            net.replay()
        for nm, want in mn.ref.items():
            if not net.unwritten(nm):
                got = host(net.tensor(nm))
                assert np.array_equal(got, want), (what, mode, nm, int(np.count_nonzero(got != want)))
                out[(mode, nm)] = got
    return out


def test_mini_net_flag_off_static_forced_autotuned():
    """flag off, static, each form forced and autotuned: identical bytes on every written edge; inner edges unwritten exactly while the
    site is on; the launch count drops by 3 per site that is on; capture / replay equals eager"""
    off = MiniNet(False)
    assert not fire_sites(off.net)
    check_mini(off, "flag off", 0)
    mn = MiniNet(True)
    assert mn.sites == 2 and [f for _, f in fire_sites(mn.net)] == [0, 0]      # the static rule names no 13 x 13 shape: four launches
    static = mn.net.choices()
    check_mini(mn, "static", 0)
    for code in (1, 2):
        assert [f for _, f in force(mn.net, code)] == [code, code]
        check_mini(mn, "forced form %d" % code, 2)
    i0 = fire_sites(mn.net)[0][0]      # one site on, one off
    L.check(L.load().saber_hip_net_set_choice(mn.net.h, i0, mn.net.choices()[i0] & ~(15 << 24)))
    check_mini(mn, "first site off", 1)
    mn.net.set_choices(static)
    assert mn.net.choices() == static
    mn.net.autotune(iters=2)
    check_mini(mn, "autotuned", sum(1 for _, f in fire_sites(mn.net) if f))
    tuned = mn.net.choices()
    fresh = MiniNet(True)
    fresh.net.set_choices(tuned)      # the choice words round-trip the forms
    assert fresh.net.choices() == tuned
    check_mini(fresh, "restored", sum(1 for _, f in fire_sites(fresh.net) if f))
    bad = tuned[i0] & ~(15 << 24) | (5 << 24)      # a code without a form: refused, nothing changes
    assert L.load().saber_hip_net_set_choice(fresh.net.h, i0, bad) != 0 and fresh.net.choices() == tuned
    fresh.net.compact()
    fresh.net.tensor("x").copy_(dev(fresh.x))
    fresh.net.run()
    assert np.array_equal(host(fresh.net.tensor("f2_y")), fresh.ref["f2_y"])


@pytest.mark.parametrize("batch,hw", [(1, 224), (2, 63)])
def test_squeezenet_with_the_fire_flag(batch, hw):
    """squeezenet_v1_1 INT8 with fire=True: eight sites; static, each form forced, autotuned - every written edge bit for bit"""
    from anakin_amd import workloads as W
    from tests.test_gpu_fire import run_passes
    model = W.build_model("squeezenet_v1_1")
    fw = W.framework_model(model, "int8")
    x = W.make_input(batch, hw=hw)
    scales = W.calibrate(model, x)
    ref = FU.run_int8(fw, scales, x)
    plain = W.build_int8_net(fw, dict(scales), batch, hw=hw)
    assert plain.fired == 0 and not fire_sites(plain)
    net = W.build_int8_net(fw, dict(scales), batch, hw=hw, fire=True)
    assert net.fired == 8 and len(fire_sites(net)) == 8
    n_on = sum(1 for _, f in fire_sites(net) if f)      # the static rule: fire2 .. fire5 at 224 x 224 x batch 1 (profiles/fire/README.md), nothing at 63 x 63
    assert n_on == (4 if (batch, hw) == (1, 224) else 0) and net.num_launches() == plain.num_launches() - 3 * n_on
    if not n_on:
        assert [net.op_name(i) for i in range(net.num_ops())] == [plain.op_name(i) for i in range(plain.num_ops())]
    run_passes(net, x, ref, (batch, hw, "fire static"), 38 - 3 * n_on)
    for code in (1, 2):
        force(net, code)
        assert net.num_launches() == plain.num_launches() - 24
        assert sum(1 for nm in net.tensors if nm.startswith("fire") and net.unwritten(nm)) == 24
        run_passes(net, x, ref, (batch, hw, "fire forced %d" % code), 38 - 24)
    net.autotune(iters=2)
    run_passes(net, x, ref, (batch, hw, "fire autotuned"), 38 - 24)


def test_flag_forms_no_site_on_a_net_without_fire_modules():
    from anakin_amd import workloads as W
    model = W.build_model("resnet50")
    fw = W.framework_model(model, "int8")
    x = W.make_input(1)
    scales = W.calibrate(model, x)
    a = W.build_int8_net(fw, dict(scales), 1)
    b = W.build_int8_net(fw, dict(scales), 1, fire=True)
    assert b.fired == 0
    assert [a.op_name(i) for i in range(a.num_ops())] == [b.op_name(i) for i in range(b.num_ops())] and a.choices() == b.choices()
