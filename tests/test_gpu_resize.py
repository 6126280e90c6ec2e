"""The resize op on the GPU (anakin_amd/csrc/resize.hip): every mode x every accepted form on the geometries of tests/resize_util.py, all
layout pairs, `==` against resize_ref (the float32 restatement of the reference that tests/test_resize_cpu.py ties to the reference's own
recorded outputs); the fused sum against the two launches bit for bit; guard bands; every form beyond one grid stride; an FPN-style list
through the executor with the resize + sum site (flag 131072) on, off and where it must decline; the Saber-side class through the stand-in
C++ driver."""
import os
import subprocess

import numpy as np
import pytest
import torch

from anakin_amd import lib as L
from anakin_amd import saber as S
from oracle import oracle as O
from tests import guard_util as GU
from tests import resize_util as RU

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["resize_direct_f32", "resize_rows_f32", "resize_x2_f32"]
X2 = {"x2_4x6_m1", "x2_4x6_m3", "x2_3x5_m1", "x2_3x5_m3"}      # integer x2 in modes 1 and 3: the cases form 2 accepts (NHWC, C % 4 == 0)
RESIZE_SUM = 131072
GEOM = sorted(RU.geometry_cases(1, 1))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def nhwc(a):
    return np.ascontiguousarray(a.transpose(0, 2, 3, 1))


def lay(a_nchw, layout):
    return np.ascontiguousarray(a_nchw) if layout == L.NCHW else nhwc(a_nchw)


def unlay(a, layout):
    return a if layout == L.NCHW else a.transpose(0, 3, 1, 2)


def _op(cs, layout=L.NHWC):
    return S.SaberResize((cs["n"], cs["c"], cs["h"], cs["w"]), cs["mode"], cs["scale_h"], cs["scale_w"], cs["out_h"], cs["out_w"], layout)


def _run(op, x_nchw, form):
    """the op's output as NCHW, whatever its layouts"""
    op.set_tile(form)
    assert op.algo() == NAMES[form] and op.tile() == form
    y = op.new_output()
    y.fill_(float("nan"))
    op.run(dev(lay(x_nchw, op.desc.in_layout)), y)
    return unlay(host(y), op.desc.out_layout)


def same(a, b):
    return GU.same_bytes(np.ascontiguousarray(a), np.ascontiguousarray(b))


@pytest.mark.parametrize("name", GEOM)
def test_every_mode_and_form_equals_resize_ref(name):
    """N in {1, 3}; C in {3, 5}: form 0 alone, all four layout pairs; C in {4, 8, 12, 36}: NHWC, forms 0 and 1, and form 2 on the x2 cases"""
    for n in (1, 3):
        for c in (3, 5, 4, 8, 12, 36):
            cs = RU.geometry_cases(n, c)[name]
            x = RU.make(cs, np.random.default_rng(RU.seed_of(name) + 7 * n + c))
            want = RU.resize_ref(x, cs)
            if c % 4:
                for layout in ((L.NHWC, L.NHWC), (L.NHWC, L.NCHW), (L.NCHW, L.NHWC), (L.NCHW, L.NCHW)):
                    op = _op(cs, layout)
                    assert op.forms() == [0] and op.out_shape() == lay(want, layout[1]).shape
                    assert same(_run(op, x, 0), want), (name, n, c, layout)
            else:
                op = _op(cs)
                assert op.forms() == ([0, 1, 2] if name in X2 else [0, 1]), (name, op.forms())
                for f in op.forms():
                    assert same(_run(op, x, f), want), (name, n, c, NAMES[f])
                for layout in ((L.NHWC, L.NCHW), (L.NCHW, L.NHWC), (L.NCHW, L.NCHW)):
                    assert _op(cs, layout).forms() == [0]


def test_set_tile_of_an_ineligible_form_is_refused():
    cs = RU.geometry_cases(1, 6)["x2_4x6_m3"]
    op = _op(cs)
    assert op.forms() == [0] and op.algo() == NAMES[0]
    with pytest.raises(L.SaberHipError):
        op.set_tile(1)
    assert op.tile() == 0 and op.algo() == NAMES[0]
    op = _op(RU.geometry_cases(1, 8)["x2_4x6_m3"])
    assert op.forms() == [0, 1, 2]
    op.set_tile(2)
    for f in (3, -1, 7):
        with pytest.raises(L.SaberHipError):
            op.set_tile(f)
    assert op.tile() == 2 and op.algo() == NAMES[2]
    # form 2 is for an integer x2 in modes 1 and 3 alone
    for nm in ("x2_4x6_m0", "x2_4x6_m2", "x8_3x5_m1", "up_5x7_11x13_m3", "same_7x7_m1"):
        op = _op(RU.geometry_cases(1, 8)[nm])
        op.set_tile(1)
        with pytest.raises(L.SaberHipError):
            op.set_tile(2)
        assert op.forms() == [0, 1] and op.tile() == 1 and op.algo() == NAMES[1]


def test_an_eight_bit_descriptor_is_unimplemented():
    for dt in (L.S8, L.U8):
        with pytest.raises(L.SaberHipError) as e:
            S.SaberResize((1, 4, 4, 4), RU.NEAREST_ALIGN, out_h=8, out_w=8, dtype=dt)
        assert e.value.status == -3, e.value      # SABER_HIP_UNIMPL


SUM_CASES = ["x2_4x6_m3", "x2_3x5_m1", "up_5x7_11x13_m0", "scale2.5_m2", "down_9x11_4x5_m1"]


@pytest.mark.parametrize("name", SUM_CASES)
def test_run_sum_equals_run_followed_by_the_eltwise_launch(name):
    """every form (C = 5: form 0 in NCHW and NHWC; C = 8: both forms), relu on and off, coefficients (1, 1) and (0.5, -1.25), the eltwise
    launch with the resized tensor as its first and as its second operand: all the same bytes, and those of the numpy restatement"""
    for c, layouts in ((5, (L.NHWC, L.NCHW)), (8, (L.NHWC,))):
        cs = RU.geometry_cases(3, c)[name]
        rng = np.random.default_rng(RU.seed_of(name) + c)
        x = RU.make(cs, rng)
        r_ref = RU.resize_ref(x, cs)
        b = rng.standard_normal(r_ref.shape).astype(np.float32)
        for layout in layouts:
            op = _op(cs, layout)
            xd, bd = dev(lay(x, layout)), dev(lay(b, layout))
            for f in op.forms():
                op.set_tile(f)
                r = op.run(xd, op.new_output())
                assert same(unlay(host(r), layout), r_ref)
                for c0, c1 in ((1.0, 1.0), (0.5, -1.25)):
                    for relu in (False, True):
                        two_a = host(S.eltwise_sum(r, bd, (c0, c1), relu))
                        two_b = host(S.eltwise_sum(bd, r, (c1, c0), relu))
                        y = op.new_output()
                        y.fill_(float("nan"))
                        one = host(op.run_sum(xd, bd, y, c0, c1, relu))
                        what = (name, c, layout, NAMES[f], c0, c1, relu)
                        assert same(one, two_a) and same(one, two_b), what
                        assert same(unlay(one, layout), RU.sum_ref(r_ref, b, c0, c1, relu)), what


@pytest.mark.parametrize("name", ["x2_3x5_m3", "x2_4x6_m1", "up_5x7_11x13_m1", "scale2.5_m2", "x8_3x5_m0", "down_9x11_4x5_m2", "to_1x1_m1"])
def test_every_form_between_guard_bands(name):
    """nothing is written outside the output, the inputs keep their bytes and the output does not depend on what lies next to the tensors -
    for the plain launch and the fused sum of every form"""
    cs = RU.geometry_cases(2, 12)[name]
    rng = np.random.default_rng(RU.seed_of(name) + 3)
    x = RU.make(cs, rng)
    want = RU.resize_ref(x, cs)
    b = rng.standard_normal(want.shape).astype(np.float32)
    want_sum = RU.sum_ref(want, b, 0.5, -1.25, True)
    op = _op(cs)
    oshape = op.out_shape()

    def plain(inputs, outputs, ws_bytes):
        T = {n: dev(a) for n, a in inputs.items()}
        for n, (shape, dt, prev) in outputs.items():
            T[n] = torch.full(shape, float(GU.SENTINEL), dtype=torch.float32, device="cuda")
        return T, None

    for f in op.forms():
        op.set_tile(f)
        what = "%s %s" % (name, NAMES[f])
        out = GU.run_guarded({"x": nhwc(x)}, {"y": (oshape, np.float32, None)}, lambda T, ws: op.run(T["x"], T["y"]), plain=plain, what=what)
        GU.assert_no_sentinel_run(out["y"], what)
        assert same(out["y"].transpose(0, 3, 1, 2), want), what
        out = GU.run_guarded({"x": nhwc(x), "b": nhwc(b)}, {"y": (oshape, np.float32, None)},
                             lambda T, ws: op.run_sum(T["x"], T["b"], T["y"], 0.5, -1.25, True), plain=plain, what=what + " + sum")
        assert same(out["y"].transpose(0, 3, 1, 2), want_sum), what + " + sum"


@pytest.mark.parametrize("form", [0, 1])
def test_beyond_one_grid_stride(form):
    """C = 4, one pixel -> one output image of 1 460 x 1 460: 8.5 M output elements (form 0) and 2.13 M float4 lanes (form 1) against a grid
    capped at 8 192 workgroups of 256 lanes = 2 097 152 lanes: the loop's second trip. RESIZE_CUSTOM from one pixel: both neighbours read
    as 0, so every output pixel is w00 times the input's four channels."""
    cs = RU.case(1, 4, 1, 1, RU.RESIZE_CUSTOM, 1460, 1460)
    x = np.array([1.5, -2.25, 3.0, 0.125], np.float32).reshape(1, 4, 1, 1)
    op = _op(cs)
    op.set_tile(form)
    y = op.new_output()
    y.fill_(float("nan"))
    op.run(dev(nhwc(x)), y)
    torch.cuda.synchronize()
    # mode 2 from one pixel: f = o / 1460, both neighbours read as 0 -> y = w00 * x with w00 = float((1 - fh) * (1 - fw)); compared on the device
    fr = torch.from_numpy(RU.axis_table(RU.RESIZE_CUSTOM, 1, 1460, 0.0, True)[2].astype(np.float64)).cuda()
    w00 = ((1.0 - fr)[:, None] * (1.0 - fr)[None, :]).to(torch.float32)
    want = w00[None, :, :, None] * dev(x.reshape(1, 1, 1, 4))
    assert y.shape == (1, 1460, 1460, 4) and bool(torch.equal(y, want))
    assert same(host(y[0, ::211, ::97]).transpose(2, 0, 1)[None], RU.resize_ref(x, cs)[:, :, ::211, ::97])


def test_x2_form_beyond_one_grid_stride():
    """form 2's lanes are INPUT float4s: C = 4, 1 460 x 1 460 -> 2 920 x 2 920 bilinear (mode 1, whose x2 table is exact at any size) is
    2.13 M lanes against 2 097 152 per stride. Forms 1 and 0 run the same case (8.5 M lanes / 34 M elements) and all three are compared on the
    device; the top and bottom 8 output rows against resize_ref on the 6 input rows they read (x2 is translation invariant)."""
    n_in = 1460
    cs = RU.case(1, 4, n_in, n_in, RU.BILINEAR_NO_ALIGN, 2 * n_in, 2 * n_in)
    x = np.random.default_rng(2920).standard_normal((1, 4, n_in, n_in)).astype(np.float32)
    op = _op(cs)
    assert op.forms() == [0, 1, 2]
    xd = dev(nhwc(x))
    ys = []
    for f in (2, 1, 0):
        op.set_tile(f)
        y = op.new_output()
        y.fill_(float("nan"))
        ys.append(op.run(xd, y))
    torch.cuda.synchronize()
    assert bool(torch.equal(ys[0], ys[1])) and bool(torch.equal(ys[0], ys[2]))
    crop = RU.case(1, 4, 6, n_in, RU.BILINEAR_NO_ALIGN, 12, 2 * n_in)
    assert same(host(ys[0][:, :8]).transpose(0, 3, 1, 2), RU.resize_ref(x[:, :, :6], crop)[:, :, :8])
    assert same(host(ys[0][:, -8:]).transpose(0, 3, 1, 2), RU.resize_ref(x[:, :, -6:], crop)[:, :, -8:])


# ---- the op inside the executor -------------------------------------------------------------------------------------------------------------
def _conv(shape, p):
    w, b, stride, pad, relu = p
    return S.SaberConv2D(False).init(shape, S.ConvParam(w, b, 1, (pad, pad), (stride, stride), (1, 1), relu), L.F32, L.F32, in_layout=L.NHWC, out_layout=L.NHWC)


_FPN_REF = {}


def _fpn_ref(n):
    """the walk with the oracle's FP32 conv and resize_ref, once per batch size"""
    if n not in _FPN_REF:
        x, layers = RU.fpn_list(n)
        ref = {"x": x}
        for kind, name, ins, p in layers:
            if kind == "conv":
                ref[name] = O.conv_f32_nchw(ref[ins[0]], p[0], p[1], p[4], (p[3], p[3]), (p[2], p[2]))
            elif kind == "resize":
                ref[name] = RU.resize_ref(ref[ins[0]], p)
            else:
                ref[name] = RU.sum_ref(ref[ins[0]], ref[ins[1]], p[0], p[1], p[2])
        for v in ref.values():
            v.setflags(write=False)
        _FPN_REF[n] = ref
    return _FPN_REF[n]


def _fpn(n, flags=0):
    x, layers = RU.fpn_list(n)
    ref = _fpn_ref(n)
    net = S.Net()
    for nm, v in ref.items():
        nn, cc, hh, ww = v.shape
        net.add_tensor(nm, (nn, hh, ww, cc), L.F32)
    idx = {}
    for kind, name, ins, p in layers:
        if kind == "conv":
            idx[name] = net.add_conv(_conv(ref[ins[0]].shape, p), ins[0], name)
        elif kind == "resize":
            idx[name] = net.add_resize(_op(p), ins[0], name)
        else:
            idx[name] = net.add_eltwise_f32(ref[name].size, p[0], p[1], p[2], ins[0], ins[1], name)
    formed = net.optimize(flags) if flags else 0
    net.finalize()
    return net, ref, idx, formed


def _fill(net, ref):
    for nm in ref:
        net.tensor(nm).fill_(float("nan"))
    net.tensor("x").copy_(dev(nhwc(ref["x"])))


def _edges(net, ref, names=None):
    return {nm: host(net.tensor(nm)).transpose(0, 3, 1, 2).copy() for nm in (names or [k for k in ref if k != "x"])}


def _close(got, ref, what):
    for nm, g in got.items():
        want = np.asarray(ref[nm], np.float64)
        d = np.abs(g.astype(np.float64) - want)
        e_max = float(d.max() / max(np.abs(want).max(), 1e-30))
        e_el = float((d / (np.abs(want) + np.abs(want).mean() + 1e-30)).max())
        assert e_max <= 1e-4 and e_el <= 1e-4, (what, nm, e_max, e_el)


@pytest.mark.parametrize("n", [1, 3])
def test_fpn_list_eager_replayed_and_autotuned(n):
    net, ref, idx, _ = _fpn(n)
    assert net.num_ops() == net.num_launches() == 12
    for nm in ("u3", "u2", "out"):
        i = idx[nm]
        assert net.op_name(i).startswith("resize:resize_") and net.choices()[i] >> 16 == 19
        nbytes, flops = net.op_work(i)
        src = [ins[0] for kind, name, ins, p in RU.fpn_list(n)[1] if name == nm][0]
        assert nbytes == 4.0 * (ref[src].size + ref[nm].size) and flops == 7.0 * ref[nm].size
    _fill(net, ref)
    net.run()
    _close(_edges(net, ref), ref, "eager")
    _fill(net, ref)
    net.capture()
    net.replay()
    _close(_edges(net, ref), ref, "replayed")
    # one op on its own; every form through the choice word; the bits do not depend on the form
    i = idx["u2"]
    first = None
    for form in (2, 1, 0):
        ch = net.choices()
        ch[i] = (19 << 16) | form
        net.set_choices(ch)
        assert net.choices()[i] == (19 << 16) | form and net.op_name(i) == "resize:" + NAMES[form]
        net.tensor("u2").fill_(float("nan"))
        net.run_op(i)
        got = _edges(net, ref, ["u2"])["u2"]
        assert same(got, RU.resize_ref(_edges(net, ref, ["p2"])["p2"], RU.fpn_list(n)[1][8][3]))
        first = got if first is None else first
        assert same(got, first)
    ch = net.choices()
    ch[i] = (19 << 16) | 5
    with pytest.raises(L.SaberHipError):
        net.set_choices(ch)
    assert net.op_name(i) == "resize:" + NAMES[0]
    _fill(net, ref)
    net.run()
    net.autotune(3)
    tuned = net.choices()
    for nm in ("u3", "u2", "out"):
        assert tuned[idx[nm]] >> 16 == 19 and (tuned[idx[nm]] & 0xff) in (0, 1, 2)
        assert net.op_name(idx[nm]) == "resize:" + NAMES[tuned[idx[nm]] & 0xff]
    _fill(net, ref)
    net.capture()
    net.replay()
    _close(_edges(net, ref), ref, "autotuned, replayed")


@pytest.mark.parametrize("n", [1, 3])
def test_fpn_list_with_the_resize_sum_sites(n):
    """flag 131072: two sites, both merged edges unwritten, two launches fewer; with SABER_HIP_NET_REPRODUCIBLE_FP32 every surviving edge has
    the bytes of the net without the flag - eagerly, replayed and autotuned"""
    base, ref, idx, _ = _fpn(n, 8192)
    _fill(base, ref)
    base.run()
    plain = _edges(base, ref)
    _close(plain, ref, "without the flag")
    net, ref, idx, formed = _fpn(n, 8192 | RESIZE_SUM)
    assert formed == 2 and net.num_ops() == 12 and net.num_launches() == 10
    assert [net.unwritten(t) for t in ("u3", "u2", "p2", "p1", "out")] == [True, True, False, False, False]
    for nm, e in (("u3", "p2"), ("u2", "p1")):
        i = idx[nm]
        assert net.op_name(i).endswith("+sum") and net.op_name(idx[e]) == "eltwise_sum_f32 (in the resize launch)"
        assert net.choices()[i] & 0x100
        src = [ins[0] for kind, name, ins, p in RU.fpn_list(n)[1] if name == nm][0]
        assert net.op_work(i) == (4.0 * (ref[src].size + 2 * ref[nm].size), 7.0 * ref[nm].size) and net.op_work(idx[e]) == (0.0, 0.0)
    survivors = [k for k in ref if k not in ("x", "u3", "u2")]

    def check(what):
        got = _edges(net, ref, survivors)
        _close(got, ref, what)
        for nm in survivors:
            assert same(got[nm], plain[nm]), (what, nm)

    _fill(net, ref)
    net.run()
    check("eager")
    assert bool(torch.isnan(net.tensor("u3")).all()) and bool(torch.isnan(net.tensor("u2")).all())      # reported unwritten and indeed untouched
    _fill(net, ref)
    net.capture()
    net.replay()
    check("replayed")
    _fill(net, ref)
    net.run()
    net.autotune(3)
    on = [bool(c & 0x100) for c in (net.choices()[idx["u3"]], net.choices()[idx["u2"]])]
    assert net.num_launches() == 12 - sum(on) and [net.unwritten("u3"), net.unwritten("u2")] == on
    _fill(net, ref)
    net.run()
    got = _edges(net, ref, survivors)
    for nm in survivors:
        assert same(got[nm], plain[nm]), ("autotuned", nm)
    # the decision travels in the choice word: off and on again
    ch = net.choices()
    for nm in ("u3", "u2"):
        ch[idx[nm]] &= ~0x100
    net.set_choices(ch)
    assert net.num_launches() == 12 and not net.unwritten("u3") and net.op_name(idx["p2"]) == "eltwise_sum_f32"
    _fill(net, ref)
    net.run()
    got = _edges(net, ref)
    for nm in got:
        assert same(got[nm], plain[nm]), ("sites off", nm)
    for nm in ("u3", "u2"):
        ch[idx[nm]] |= 0x100
    net.set_choices(ch)
    assert net.num_launches() == 10 and net.unwritten("u3") and net.unwritten("u2")


def _small_list(kind):
    """resize 4x4 -> 8x8 (nearest, C = 8) and an eltwise, arranged so that flag 131072 must decline"""
    n, c = 2, 8
    cs = RU.case(n, c, 4, 4, RU.NEAREST_ALIGN, 8, 8)
    rng = np.random.default_rng(11)
    x = RU.make(cs, rng)
    b = rng.standard_normal((n, c, 8, 8)).astype(np.float32)
    net = S.Net()
    net.add_tensor("x", (n, 4, 4, c), L.F32)
    for nm in ("b", "r", "y", "z"):
        net.add_tensor(nm, (n, 8, 8, c), L.F32)
    count = n * c * 64
    ref = {"x": x, "b": b, "r": RU.resize_ref(x, cs)}
    if kind == "second_reader":
        net.add_resize(_op(cs), "x", "r")
        net.add_eltwise_f32(count, 1.0, 1.0, False, "r", "b", "y")
        net.add_eltwise_f32(count, 0.5, 2.0, True, "b", "r", "z")
        ref["y"] = RU.sum_ref(ref["r"], b, 1.0, 1.0, False)
        ref["z"] = RU.sum_ref(b, ref["r"], 0.5, 2.0, True)
    elif kind == "not_next":
        net.add_resize(_op(cs), "x", "r")
        net.add_eltwise_f32(count, 0.5, 2.0, True, "b", "b", "z")
        net.add_eltwise_f32(count, 1.0, 1.0, False, "r", "b", "y")
        ref["z"] = RU.sum_ref(b, b, 0.5, 2.0, True)
        ref["y"] = RU.sum_ref(ref["r"], b, 1.0, 1.0, False)
    elif kind == "side_lane":
        net.add_resize(_op(cs), "x", "r")
        net.add_eltwise_f32(count, 1.0, 1.0, False, "r", "b", "y")
        i = net.add_eltwise_f32(count, 0.5, 2.0, True, "b", "b", "z")
        net.set_lane(i, 1)
        ref["y"] = RU.sum_ref(ref["r"], b, 1.0, 1.0, False)
        ref["z"] = RU.sum_ref(b, b, 0.5, 2.0, True)
    else:      # own_input: an identity resize whose eltwise sums it with the resize's own input
        cs = RU.case(n, c, 8, 8, RU.BILINEAR_NO_ALIGN, 8, 8)
        net.add_resize(_op(cs), "b", "r")
        net.add_eltwise_f32(count, 1.0, -0.5, False, "r", "b", "y")
        ref["r"] = RU.resize_ref(b, cs)
        ref["y"] = RU.sum_ref(ref["r"], b, 1.0, -0.5, False)
    return net, ref


@pytest.mark.parametrize("kind", ["second_reader", "not_next", "side_lane", "own_input"])
def test_lists_where_the_flag_must_decline(kind):
    outs = []
    for flags in (0, RESIZE_SUM):
        net, ref = _small_list(kind)
        formed = net.optimize(flags) if flags else 0
        assert formed == 0
        net.finalize()
        assert net.num_launches() == net.num_ops() and not net.unwritten("r")
        for nm in ("r", "y", "z"):
            net.tensor(nm).fill_(float("nan"))
        net.tensor("x").copy_(dev(nhwc(ref["x"])))
        net.tensor("b").copy_(dev(nhwc(ref["b"])))
        net.run()
        got = {nm: host(net.tensor(nm)).transpose(0, 3, 1, 2).copy() for nm in ref if nm not in ("x", "b")}
        for nm in got:
            assert same(got[nm], ref[nm]), (kind, flags, nm)
        outs.append(got)
    for nm in outs[0]:
        assert same(outs[0][nm], outs[1][nm])


def test_resize_is_recorded_by_the_op_list_capture():
    cs = RU.geometry_cases(2, 8)["up_5x7_11x13_m1"]
    x = RU.make(cs, np.random.default_rng(9))
    op = _op(cs)
    xd, y = dev(nhwc(x)), op.new_output()
    y.fill_(123.0)
    with S.Capture() as cap:
        op.run(xd, y)
    assert float(host(y).min()) == 123.0 == float(host(y).max())      # recorded, not launched
    net = cap.net
    assert net.num_ops() == 1 and net.op_name(0) == "resize:" + op.algo()
    net.bind(net.tensor_of_ptr(y), y)
    net.finalize()
    net.run()
    assert same(host(y).transpose(0, 3, 1, 2), RU.resize_ref(x, cs))


def test_saber_resize_through_the_stand_in_cpp_driver():
    """tests/cpp/test_saber_resize.cpp: SaberResize<MI355X, AK_FLOAT> init -> dispatch under the stand-in Saber headers"""
    exe = os.path.join(ROOT, "tests", "cpp", "test_saber_resize.bin")
    assert os.path.exists(exe), "tests/cpp/test_saber_resize.bin is missing: run __graft_entry__.build()"
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = os.pathsep.join([os.path.join(ROOT, "anakin_amd"), os.path.join(ROOT, "oracle"), env.get("LD_LIBRARY_PATH", "")])
    p = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0 and "resize cases bit for bit" in p.stdout, p.stdout[-3000:] + p.stderr[-2000:]
