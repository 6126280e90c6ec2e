"""Unequal eltwise coefficients, coeff_conv != coeff_res, on random data through the fused forms the tie probes cannot reach: the XCD stage
(stage_xcd.hip), conv + global pooling (conv1x1_gpool.hip), the inverted-residual block's project eltwise (conv_ir.hip) and the executor's
conv + eltwise fusion (saber_hip_net_optimize flag 1, which maps the eltwise op's (coeff_a, coeff_b) onto (conv, residual) by the operand
the conv produces). Every case against the oracle with (c, -c / 2) and (c / 2, c); before anything is launched the oracle alone shows that
a swapped pair and the conv's coefficient used for both would each change at least a quarter of the bytes (tests/block_table.py)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from anakin_amd import lib as L  # noqa: E402
from anakin_amd import saber as S  # noqa: E402
from oracle import oracle as O  # noqa: E402
from tests import block_table as BT  # noqa: E402
from tests import ir_util as IU  # noqa: E402
from tests import tail_util as T  # noqa: E402
from tests import test_gpu_ir as TIR  # noqa: E402
from tests import test_gpu_stage as TS  # noqa: E402

dev, host = TS.dev, TS.host
PAIRS = BT.UNEQUAL


@pytest.fixture(scope="module", autouse=True)
def _device():
    L.require_device()


def test_xcd_stage_res5_unequal_coefficients_equals_the_ops_and_oracle():
    """res5 at batch 1 (the smallest of tests/test_gpu_stage.py): the three blocks' eltwise pairs are (c, -c / 2), (c / 2, c), (c, -c / 2);
    the one launch == the ops one by one == the oracle walk, three launches"""
    N = 1
    rng = np.random.default_rng(901)
    keep = {}
    ph, nt = TS.res5(rng, N, pairs=PAIRS, keep=keep)
    x0 = rng.integers(-128, 128, (N, 7, 7, 1024)).astype(np.int8)
    ref, n_elt = [x0] + [None] * (nt - 1), 0
    for c, i, o, r in ph:
        q = keep[id(c)]
        ws = O.weight_scales(q["w"])
        bp, sc = O.conv_i8_prepare(ws, q["b"], q["s_in"], q["s_out"], q["idt"], q["odt"])
        y = O.conv_i8(ref[i], O.quant_weights(q["w"], ws), bp, sc, q["odt"], q["relu"], (q["k"] // 2,) * 2)
        if r >= 0:
            c0, c1 = q["coeff"]
            print("res5 eltwise %d: %s" % (n_elt, BT.coeff_conditions(y, ref[r], q["s_out"], q["s_res"], c0, c1, True, "res5 eltwise %d" % n_elt)))
            y = O.eltwise_i8(y, ref[r], q["s_out"], q["s_res"], c0, c1, True)
            n_elt += 1
        ref[o] = y
    assert n_elt == 3
    want = [dev(x0)] + [None] * (nt - 1)
    for c, i, o, r in ph:
        want[o] = c.new_output()
        c.dispatch(want[i], want[o], None if r < 0 else want[r])
        assert np.array_equal(host(want[o]), ref[o]), ("op", o, c.algo())
    stage = S.SaberStage(ph)
    for rep in range(3):
        got = [dev(x0)] + [torch.full_like(t, 77) for t in want[1:]]
        stage.dispatch(got)
        stage.status()
        for k in range(1, nt):
            assert np.array_equal(host(got[k]), ref[k]), ("slot", k, "launch", rep)


@pytest.mark.parametrize("pair", PAIRS)
@pytest.mark.parametrize("epi", T.GPOOL_EPILOGUES[:2], ids=[e[0] for e in T.GPOOL_EPILOGUES[:2]])
def test_conv1x1_with_global_pooling_unequal_coefficients(epi, pair):
    H, W, N, cout = 5, 3, 1, T.GPOOL_COUTS[1]
    wq, ws, b, xs, rs = T.gpool_case(H, W, N, cout, epi)
    d = {}
    want, want_pool = T.gpool_oracle(wq, ws, b, xs[0], rs[0], epi, pair, d)
    cc = T.gpool_coeff(pair)
    print("gpool %s %s: %s" % (epi[0], pair, BT.coeff_conditions(d["t1"], rs[0], T.S_OUT, T.S_RES, cc[0], cc[1], epi[2], "gpool", want)))
    conv = T.gpool_op(N, H, W, cout, wq, ws, b, epi, pair)
    assert conv.algo() == "imgres1x1_i8_64ch+gpool", conv.algo()
    y = conv.new_output()
    yp = torch.empty((N, 1, 1, cout), dtype=y.dtype, device="cuda")
    y.fill_(77)
    yp.fill_(55)
    conv.dispatch_gpool(dev(xs[0]), y, yp, dev(rs[0]))
    assert np.array_equal(host(y), want), conv.algo()
    assert np.array_equal(host(yp), want_pool), conv.algo()


@pytest.mark.parametrize("pair", PAIRS)
@pytest.mark.parametrize("vi", [0, 1], ids=["elt", "elt_relu"])
def test_inverted_residual_project_eltwise_unequal_coefficients(vi, pair):
    """geometry "a" (16 -> 96 -> 16 on 5 x 7, two images): the block's three launches and every one-launch form against the oracle"""
    cs = IU.case("a", vi, pair=pair)
    assert cs.res and cs.coeffs[0] != cs.coeffs[1]
    print("ir a/%d %s: %s" % (vi, pair, BT.coeff_conditions(cs.p, cs.x, cs.p_scale, IU.IN_SCALE, cs.coeffs[0], cs.coeffs[1], bool(cs.e_relu), "ir", cs.y)))
    TIR.run_case(cs)


# ---- the executor's conv + eltwise fusion ------------------------------------------------------------------------------------------------
def _net(side, flags):
    """conv 3x3 (64 -> 64, u8) -> conv 1x1 (64 -> 256, s8) -> eltwise with an external residual -> conv 1x1 (256 -> 64) at 1 x 6 x 8; the
    eltwise op takes the conv's output as operand a (side 0) or b (side 1), with different scales and (c0, c1) = (c, -c / 2)"""
    N, H, W, C, K = 1, 6, 8, 64, 256
    rng = np.random.default_rng(3300)
    x = rng.integers(0, 256, (N, H, W, C)).astype(np.uint8)
    res = rng.integers(-128, 128, (N, H, W, K)).astype(np.int8)
    s_x, s_in, s_mid, s_res, s_sum, s_out = 0.023, 0.02, 0.05, 0.043, 0.06, 0.031
    c = float(np.float32(1.0 / s_sum))
    c0, c1 = c, float(np.float32(-0.5 * c))
    net, ref = S.Net(), {"x": x, "res": res}
    net.add_tensor("x", x.shape, L.U8)
    net.add_tensor("res", res.shape, L.S8)

    def conv(name, src, cin, cout, k, relu, idt, odt, si, so):
        w = (rng.standard_normal((cout, cin, k, k)) * np.sqrt(2.0 / (cin * k * k))).astype(np.float32)
        b = (rng.standard_normal(cout) * 0.5).astype(np.float32)
        op = S.SaberConv2D(int8=True).init((N, cin, H, W), S.ConvParam(w, b, 1, (k // 2, k // 2), (1, 1), (1, 1), bool(relu)), idt, odt, si, so)
        ws = O.weight_scales(w)
        bp, sc = O.conv_i8_prepare(ws, b, si, so, idt, odt)
        ref[name] = O.conv_i8(ref[src], O.quant_weights(w, ws), bp, sc, odt, int(relu), (k // 2, k // 2))
        net.add_tensor(name, ref[name].shape, odt)
        net.add_conv(op, src, name)
    conv("t0", "x", C, C, 3, True, O.U8, O.U8, s_x, s_in)
    conv("t1", "t0", C, K, 1, False, O.U8, O.S8, s_in, s_mid)
    net.add_tensor("sum", res.shape, L.S8)
    if side == 0:
        ref["sum"] = O.eltwise_i8(ref["t1"], res, s_mid, s_res, c0, c1, True)
        net.add_eltwise_i8(res.size, s_mid, s_res, c0, c1, True, "t1", "res", "sum")
        conv_c, res_c = c0, c1
    else:
        ref["sum"] = O.eltwise_i8(res, ref["t1"], s_res, s_mid, c0, c1, True)
        net.add_eltwise_i8(res.size, s_res, s_mid, c0, c1, True, "res", "t1", "sum")
        conv_c, res_c = c1, c0
    print("net side %d: %s" % (side, BT.coeff_conditions(ref["t1"], res, s_mid, s_res, conv_c, res_c, True, "net side %d" % side, ref["sum"])))
    conv("y2", "sum", K, C, 1, True, O.S8, O.U8, s_sum, s_out)
    removed = [net.optimize(f) for f in flags]
    net.finalize()
    return net, ref, removed


@pytest.mark.parametrize("side", [0, 1], ids=["conv_is_operand_a", "conv_is_operand_b"])
def test_net_optimize_maps_unequal_eltwise_coefficients_onto_conv_and_residual(side):
    """unfused, then optimize(1) (the fused list is one op shorter), then the chain flags on top: every
    written edge equals the oracle and the unfused run. The two sides give different bytes, so an exchanged mapping shows."""
    a, b = _net(0, [])[1]["sum"], _net(1, [])[1]["sum"]
    assert (a != b).mean() >= 0.25, "the two operand orders must give different sums"
    runs = {}
    for what, flags, edges in (("unfused", [], ("t0", "t1", "sum", "y2")), ("fused", [1], ("t0", "sum", "y2")), ("chain", [1, 16 | 32], ("t0", "sum", "y2"))):
        net, ref, removed = _net(side, flags)
        if what == "unfused":
            assert net.num_ops() == 4 and net.num_launches() == 4
        elif what == "fused":
            assert removed == [1] and net.num_ops() == 3 and net.num_launches() == 3, (removed, net.num_ops())
        else:      # (both ops of a chain stay in the list; whether the chain launch is selected at this shape is the static rule's business)
            assert removed[0] == 1 and net.num_ops() == 3 and net.num_launches() <= 3, (removed, net.num_ops(), net.num_launches())
            edges = tuple(nm for nm in edges if not net.unwritten(nm))
            print("side %d, chain flags: optimize returned %s, %d launches, written edges %s" % (side, removed, net.num_launches(), edges))
        for nm in edges:
            net.tensor(nm).fill_(77)
        net.tensor("x").copy_(dev(ref["x"]))
        net.tensor("res").copy_(dev(ref["res"]))
        net.run()
        runs[what] = {nm: host(net.tensor(nm)) for nm in edges}
        for nm in edges:
            assert np.array_equal(runs[what][nm], ref[nm]), (what, nm, side, [net.op_name(i) for i in range(net.num_ops())])
    for what in ("fused", "chain"):
        for nm, v in runs[what].items():
            assert np.array_equal(v, runs["unfused"][nm]), (what, nm)
