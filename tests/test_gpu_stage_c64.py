"""The res2 stage launch (conv_stage_coop.hip: conv_stage1_c64_kernel; saber_hip_conv2d_stage_create at C = 64): a run of ResNet res2 block
chains [conv3x3 64 -> 64, conv1x1 64 -> 256 + eltwise, the next block's conv1x1 256 -> 64] as ONE persistent launch, one workgroup of four
waves per tile of 2 rows x 16 columns, four workgroups per CU, an image per XCD, the XCD-local edge barrier between two blocks.

Operator level: every block's outputs bit for bit the oracle walk's and the chain launches', on the smallest shapes that take every path
(one / two / four column tiles, ragged rows and columns, parity-word reuse with three blocks, XCD slots without an image, every XCD with
one), with u8 and s8 hand-overs, the shortcut sum with and without relu, three launches in a row on one stage object (the counters are never
reset) and the form that leaves the inner blocks' first outputs unwritten. What the stage has no kernel for is refused with
SABER_HIP_INVALID_VALUE before anything is launched.

Net level: ResNet50 INT8 at batch 1 and 8 with the res2 site switched on by its choice word - one launch fewer, the inner tensor unwritten,
every written edge of every image bit-exact against the oracle, eager and as a hipGraph - and switched off again: the parent's names,
choice words and launch count."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from anakin_amd import lib as L  # noqa: E402
from anakin_amd import saber as S  # noqa: E402
from anakin_amd import workloads as W  # noqa: E402
from oracle import oracle as O  # noqa: E402
from tests import test_gpu_stage_tail as TT  # noqa: E402

Cc, K1 = 64, 256


@pytest.fixture(scope="module", autouse=True)
def _device():
    L.require_device()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _blocks(rng, N, H, Wd, nblk, hand, res_relu, c=Cc):
    """nblk block chains [3x3 -> 1x1 expand + eltwise -> next block's 1x1 reduce] at C = c, chain i + 1 reading chain i's outputs; `hand`:
    the dtype every block hands to the next one's 3x3 conv (and the first input's); `res_relu`: relu on the shortcut sum. Returns the first
    inputs, the device ops and the oracle's two outputs per block."""
    k1 = 4 * c
    x = rng.integers(0, 256, (N, H, Wd, c)).astype(np.uint8) if hand == O.U8 else rng.integers(-128, 128, (N, H, Wd, c)).astype(np.int8)
    res = rng.integers(-128, 128, (N, H, Wd, k1)).astype(np.int8)
    ops, wants = [], []
    cur_x, cur_res = x, res
    for k in range(nblk):
        w0 = (rng.standard_normal((c, c, 3, 3)) * np.sqrt(2.0 / (9 * c))).astype(np.float32)
        b0 = (rng.standard_normal(c) * 0.5).astype(np.float32)
        w1 = (rng.standard_normal((k1, c, 1, 1)) * np.sqrt(2.0 / c)).astype(np.float32)
        b1 = (rng.standard_normal(k1) * 0.5).astype(np.float32)
        w2 = (rng.standard_normal((c, k1, 1, 1)) * np.sqrt(2.0 / k1)).astype(np.float32)
        b2 = (rng.standard_normal(c) * 0.5).astype(np.float32)
        s_x, s_in, s_mid, s_res, s_sum, s_out = 0.023 + 0.001 * k, 0.02, 0.05, 0.043 + 0.002 * k, 0.06, 0.031
        cf = 1.0 / s_sum
        relu2 = 1 if hand == O.U8 else 0
        ws0 = O.weight_scales(w0)
        bp0, sc0 = O.conv_i8_prepare(ws0, b0, s_x, s_in, hand, O.U8)
        c0 = S.SaberConv2D(int8=True).init((N, c, H, Wd), S.ConvParam(w0, b0, 1, (1, 1), (1, 1), (1, 1), True), hand, O.U8, s_x, s_in)
        pa = S.ConvParam(w1, b1, 1, (0, 0), (1, 1), (1, 1), False)
        pa.res_mode, pa.res_relu, pa.sum_scale, pa.coeff, pa.scale_res = L.RES_ELTWISE, bool(res_relu), 1.0, (cf, cf), s_res
        ca = S.SaberConv2D(int8=True).init((N, c, H, Wd), pa, O.U8, O.S8, s_in, s_mid)
        cb = S.SaberConv2D(int8=True).init((N, k1, H, Wd), S.ConvParam(w2, b2, 1, (0, 0), (1, 1), (1, 1), bool(relu2)), O.S8, hand, s_sum, s_out)
        ops.append((c0, ca, cb))
        t0 = O.conv_i8(cur_x, O.quant_weights(w0, ws0), bp0, sc0, O.U8, 1, (1, 1))
        ws1 = O.weight_scales(w1)
        bp1, sc1 = O.conv_i8_prepare(ws1, b1, s_in, s_mid, O.U8, O.S8)
        t1 = O.conv_i8(t0, O.quant_weights(w1, ws1), bp1, sc1, O.S8, 0)
        want1 = O.eltwise_i8(t1, cur_res, s_mid, s_res, cf, cf, bool(res_relu))
        ws2 = O.weight_scales(w2)
        bp2, sc2 = O.conv_i8_prepare(ws2, b2, s_sum, s_out, O.S8, hand)
        want2 = O.conv_i8(want1, O.quant_weights(w2, ws2), bp2, sc2, hand, relu2)
        wants.append((want1, want2))
        cur_x, cur_res = want2, want1
    return x, res, ops, wants


SHAPES = [
    (1, 6, 16, 2),      # one column tile; a middle tile row with both edges
    (2, 7, 9, 3),       # ragged rows and columns, three blocks: the parity word of block 0 is used again by block 2
    (1, 5, 24, 2),      # two column tiles, ragged
    (1, 6, 56, 2),      # four column tiles with 8 ragged columns: the workload's width
    (3, 4, 20, 2),      # five XCD slots have no image and must return
    (8, 4, 64, 2),      # every XCD holds an image
]


@pytest.mark.parametrize("hand,res_relu", [(O.U8, 1), (O.S8, 0)])
@pytest.mark.parametrize("shape", SHAPES)
def test_stage_c64_equals_the_chains_and_oracle(shape, hand, res_relu):
    """every block's y1 and y2 from the one launch == the oracle walk == the chain launches, three launches in a row; then the form with
    the inner y1 tensors skipped: y2 of every block and the last y1 identical, the skipped tensors' bytes untouched"""
    N, H, Wd, nblk = shape
    rng = np.random.default_rng(6400 + N + H + Wd + nblk + res_relu)
    x, res, ops, wants = _blocks(rng, N, H, Wd, nblk, hand, res_relu)
    chains = [S.SaberConvChain(ca, cb, conv3x3=c0) for c0, ca, cb in ops]
    y1 = [ca.new_output() for _, ca, _ in ops]
    y2 = [cb.new_output() for _, _, cb in ops]
    cx, cr = dev(x), dev(res)
    for k, ch in enumerate(chains):                  # the chains one by one
        ch.dispatch(cx, cr, y1[k], y2[k])
        assert np.array_equal(host(y1[k]), wants[k][0]) and np.array_equal(host(y2[k]), wants[k][1]), ("chain", k)
        cx, cr = y2[k], y1[k]
    stage = S.SaberChainStage(chains)
    xd, rd = dev(x), dev(res)
    for rep in range(3):                             # (the edge counters are never reset)
        for t in y1 + y2:
            t.fill_(77)
        stage.dispatch(xd, rd, y1, y2)
        for k in range(nblk):
            assert np.array_equal(host(y1[k]), wants[k][0]), ("stage y1", k, rep)
            assert np.array_equal(host(y2[k]), wants[k][1]), ("stage y2", k, rep)
    # the inner y1 tensors skipped
    for t in y1 + y2:
        t.fill_(77)
    stage.dispatch(xd, rd, [None] * (nblk - 1) + [y1[-1]], y2)
    for k in range(nblk):
        assert np.array_equal(host(y2[k]), wants[k][1]), ("skipped: y2", k)
    assert np.array_equal(host(y1[-1]), wants[-1][0]), "skipped: the last y1"
    for k in range(nblk - 1):
        assert (host(y1[k]) == 77).all(), ("skipped: y1 written", k)


def test_stage_c64_refusals():
    """W = 40 (three column tiles: arrivals per edge not a power of two), N = 9 (an image per XCD), a stride-2 3x3 conv in a block, mixed C,
    a single block, a null last y1: SABER_HIP_INVALID_VALUE, nothing launched"""
    rng = np.random.default_rng(64)

    def chains_of(ops):
        return [S.SaberConvChain(ca, cb, conv3x3=c0) for c0, ca, cb in ops]

    for N, H, Wd in ((1, 4, 40), (9, 4, 16)):
        _, _, ops, _ = _blocks(rng, N, H, Wd, 2, O.U8, 1)
        with pytest.raises(L.SaberHipError, match="stage: an image per XCD"):
            S.SaberChainStage(chains_of(ops))
    # a stride-2 3x3 conv cannot lead a conv3x3 + conv1x1 + conv1x1 chain at all (so no block of a stage holds one) ...
    _, _, ops, _ = _blocks(rng, 1, 8, 16, 2, O.U8, 1)
    _, _, sops, _ = _blocks(rng, 1, 4, 8, 1, O.U8, 1)
    w0 = (rng.standard_normal((Cc, Cc, 3, 3)) * 0.05).astype(np.float32)
    s2 = S.SaberConv2D(int8=True).init((1, Cc, 8, 16), S.ConvParam(w0, None, 1, (1, 1), (2, 2), (1, 1), True), O.U8, O.U8, 0.023, 0.02)
    with pytest.raises(L.SaberHipError, match="chain: the head must be the 3x3 pad-1 INT8 conv"):
        S.SaberConvChain(sops[0][1], sops[0][2], conv3x3=s2)
    # ... and the chain form a strided head does have - conv3x3 + conv1x1, no second 1x1 conv - is no block of a stage
    good = chains_of(ops)
    with pytest.raises(L.SaberHipError, match="stage: every block must be"):
        S.SaberChainStage([good[0], S.SaberConvChain(ops[1][1], None, conv3x3=ops[1][0])])
    # mixed C
    _, _, ops128, _ = _blocks(rng, 1, 8, 16, 1, O.U8, 1, c=128)
    with pytest.raises(L.SaberHipError, match="stage: every block must be"):
        S.SaberChainStage([good[0]] + chains_of(ops128))
    # one block
    with pytest.raises(L.SaberHipError, match="at least two blocks"):
        S.SaberChainStage(good[:1])
    # the last block's y1 is always written
    stage = S.SaberChainStage(good)
    y1 = [ca.new_output() for _, ca, _ in ops]
    y2 = [cb.new_output() for _, _, cb in ops]
    for t in y1 + y2:
        t.fill_(77)
    x = dev(np.zeros((1, 8, 16, Cc), np.uint8))
    r = dev(np.zeros((1, 8, 16, K1), np.int8))
    with pytest.raises(L.SaberHipError, match="an output pointer per block"):
        stage.dispatch(x, r, [y1[0], None], y2)
    assert all((host(t) == 77).all() for t in y1 + y2)


# ------------------------------------------------------------------------------------------------ net level
@pytest.mark.parametrize("batch", [1, 8])
def test_resnet50_net_runs_res2_as_one_launch(batch):
    hw = 224
    model, scales, x, ref = TT._resnet50(batch, hw)
    net = W.build_int8_net(model, dict(scales), batch, hw=hw, stage=True)
    # formed and OFF: no generic selector sees it, the net is the parent's
    sites = net.stages_c64()
    assert len(sites) == 1 and sites[0][1] == 2 and not sites[0][2], sites
    i0 = sites[0][0]
    assert all(s[0] != i0 for s in net.stages())
    names_off = [net.op_name(i) for i in range(net.num_ops())]
    ch_off, off = net.choices(), net.num_launches()
    unwritten_off = [nm for nm in net.tensors if net.unwritten(nm)]
    # on, by its choice word
    L.check(L.load().saber_hip_net_set_choice(net.h, i0, ch_off[i0] | (1 << 30)))
    assert net.stages_c64() == [(i0, 2, True)]
    assert net.op_name(i0) == "conv:stage_c64_2x[conv3x3+chain1x1]_2x16", net.op_name(i0)
    assert all("(in the" in net.op_name(i) for i in range(i0 + 1, i0 + 6))
    assert net.num_launches() == off - 1
    assert [nm for nm in net.tensors if net.unwritten(nm) and nm not in unwritten_off] == ["res2a"]
    TT._check_edges(net, x, ref, "res2 stage on")
    net.status()
    # a fresh net takes the decision from the whole list of words
    ch_on = net.choices()
    # off again: the parent's launches, names and words
    L.check(L.load().saber_hip_net_set_choice(net.h, i0, ch_off[i0]))
    net.set_choices(ch_off)
    assert net.stages_c64() == [(i0, 2, False)] and net.num_launches() == off and net.choices() == ch_off
    assert [net.op_name(i) for i in range(net.num_ops())] == names_off
    assert [nm for nm in net.tensors if net.unwritten(nm)] == unwritten_off
    TT._check_edges(net, x, ref, "res2 stage off again")
    if batch == 8:
        # a stage launch that did not complete (the testing aid's error word): the site falls back like any stage, the next pass is right
        net.select_stages(False)
        net.select_stages_c64(True)
        before = net.num_launches()
        L.check(L.load().saber_hip_net_inject_coop_error(net.h))
        with pytest.raises(L.SaberHipError):
            net.status()
        assert net.stages_c64() == [(i0, 2, False)] and net.num_launches() == before + 1
        net.tensor("data").copy_(torch.from_numpy(x).cuda())
        net.run()
        net.status()
        assert np.array_equal(host(net.tensor("fc1000")), ref["fc1000"].reshape(host(net.tensor("fc1000")).shape))
    if batch == 1:
        fresh = W.build_int8_net(model, dict(scales), batch, hw=hw, stage=True)
        fresh.set_choices(ch_on)
        assert fresh.choices() == ch_on and fresh.stages_c64() == [(i0, 2, True)] and fresh.num_launches() == off - 1
        fresh.select_stages_c64(False)
        assert fresh.num_launches() == off and not fresh.unwritten("res2a")
        # the generic selector leaves the site alone, both ways
        fresh.select_stages(True)
        assert fresh.stages_c64() == [(i0, 2, False)] and all(s[2] for s in fresh.stages())
        fresh.select_stages_c64(True)
        fresh.select_stages(False)
        assert fresh.stages_c64() == [(i0, 2, True)] and not any(s[2] for s in fresh.stages())
