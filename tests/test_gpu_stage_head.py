"""The res4 stage launch with a HEAD (conv_stage_coop.hip, saber_hip_conv2d_stage_create_head): in front of its blocks the persistent launch
runs the sibling pair that feeds the first block - res4a_branch1 (1x1, 512 -> 1024, s8: the shortcut, which then never leaves LDS) and
res4a_branch2a (1x1, 512 -> 256: the 3x3 conv's input, written to its own tensor and handed to the neighbouring tiles through the edge
counters). Integer sums and the pair epilogue's float sequence: every tensor the launch writes holds the bits of the operators dispatched one
by one (= the oracle's), launch after launch (its counters are never reset), with and without a tail, for ragged images, both input dtypes and
both forms of branch2a; the same stage object still runs without its head; what the kernel cannot run is refused when the stage is created;
at net level (ResNet50's framework list) the head is OFF until it is selected, the head form and the separate pair write identical edges,
eager and as a hipGraph, survive a choices() round trip and fall back together with stage and tail; and the launch neither writes nor uses a
byte outside its tensors. The head's weight-stream packer (api_chain.hip: pack_stage_head_stream) has no CPU-tier walk - a stage cannot be
created without a device - and is covered by the bit-exact comparisons here."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from anakin_amd import lib as L  # noqa: E402
from anakin_amd import saber as S  # noqa: E402
from anakin_amd import workloads as W  # noqa: E402
from oracle import oracle as O  # noqa: E402
from tests import guard_util as GU  # noqa: E402
from tests import test_gpu_stage_tail as TT  # noqa: E402

dev, host = TT.dev, TT.host


@pytest.fixture(scope="module", autouse=True)
def _device():
    L.require_device()


def _rand8(rng, shape, dt):
    return rng.integers(0, 256, shape).astype(np.uint8) if dt == O.U8 else rng.integers(-128, 128, shape).astype(np.int8)


def _conv1x1(rng, N, H, Wd, Cin, K, idt, odt, relu, s_in, s_out, x_in=None, k=1, pad=0, res=False):
    """one INT8 conv (k x k, stride 1) as a device op and - given the oracle's input - its output"""
    w = (rng.standard_normal((K, Cin, k, k)) * np.sqrt(2.0 / (Cin * k * k))).astype(np.float32)
    b = (rng.standard_normal(K) * 0.5).astype(np.float32)
    p = S.ConvParam(w, b, 1, (pad, pad), (1, 1), (1, 1), bool(relu))
    if res:
        p.res_mode, p.res_relu, p.sum_scale, p.coeff, p.scale_res = L.RES_ELTWISE, True, 1.0, (1.0, 1.0), 0.05
    op = S.SaberConv2D(int8=True).init((N, Cin, H, Wd), p, idt, odt, s_in, s_out)
    want = None
    if x_in is not None:
        ws = O.weight_scales(w)
        bp, sc = O.conv_i8_prepare(ws, b, s_in, s_out, idt, odt)
        want = O.conv_i8(x_in, O.quant_weights(w, ws), bp, sc, odt, int(bool(relu)), (pad, pad))
    return op, want


def _pair(rng, N, H, Wd, idt, bdt, xh=None):
    """the sibling pair: a = 512 -> 1024, no relu, s8 (the shortcut); b = 512 -> 256, relu / u8 or no relu / s8 (the 3x3 input)"""
    a, want_a = _conv1x1(rng, N, H, Wd, 512, 1024, idt, O.S8, False, 0.027, 0.043, xh)
    b, want_b = _conv1x1(rng, N, H, Wd, 512, 256, idt, bdt, bdt == O.U8, 0.027, 0.023, xh)
    return a, b, want_a, want_b


def _blocks_from(rng, x, res, idt, nblk, Cc=256):
    """tests/test_gpu_stage_tail.py's _res4_blocks on GIVEN first inputs (the pair's outputs): nblk block chains [3x3 -> 1x1 expand +
    eltwise(relu) -> next block's 1x1 reduce], chain i + 1 reading chain i's outputs; the last conv's output dtype alternates u8 / s8"""
    N, H, Wd, _ = x.shape
    K1 = 4 * Cc
    ops, wants = [], []
    cur_x, cur_res = x, res
    for k in range(nblk):
        w0 = (rng.standard_normal((Cc, Cc, 3, 3)) * np.sqrt(2.0 / (9 * Cc))).astype(np.float32)
        b0 = (rng.standard_normal(Cc) * 0.5).astype(np.float32)
        w1 = (rng.standard_normal((K1, Cc, 1, 1)) * np.sqrt(2.0 / Cc)).astype(np.float32)
        b1 = (rng.standard_normal(K1) * 0.5).astype(np.float32)
        w2 = (rng.standard_normal((Cc, K1, 1, 1)) * np.sqrt(2.0 / K1)).astype(np.float32)
        b2 = (rng.standard_normal(Cc) * 0.5).astype(np.float32)
        s_x, s_in, s_mid, s_res, s_sum, s_out = 0.023 + 0.001 * k, 0.02, 0.05, 0.043 + 0.002 * k, 0.06, 0.031
        c = 1.0 / s_sum
        odt2 = O.U8 if k % 2 == 0 else O.S8
        relu2 = 1 if odt2 == O.U8 else 0
        ws0 = O.weight_scales(w0)
        bp0, sc0 = O.conv_i8_prepare(ws0, b0, s_x, s_in, idt, O.U8)
        t0 = O.conv_i8(cur_x, O.quant_weights(w0, ws0), bp0, sc0, O.U8, 1, (1, 1))
        ws1 = O.weight_scales(w1)
        bp1, sc1 = O.conv_i8_prepare(ws1, b1, s_in, s_mid, O.U8, O.S8)
        t1 = O.conv_i8(t0, O.quant_weights(w1, ws1), bp1, sc1, O.S8, 0)
        want1 = O.eltwise_i8(t1, cur_res, s_mid, s_res, c, c, True)
        ws2 = O.weight_scales(w2)
        bp2, sc2 = O.conv_i8_prepare(ws2, b2, s_sum, s_out, O.S8, odt2)
        want2 = O.conv_i8(want1, O.quant_weights(w2, ws2), bp2, sc2, odt2, relu2)
        c0 = S.SaberConv2D(int8=True).init((N, Cc, H, Wd), S.ConvParam(w0, b0, 1, (1, 1), (1, 1), (1, 1), True), idt, O.U8, s_x, s_in)
        pa = S.ConvParam(w1, b1, 1, (0, 0), (1, 1), (1, 1), False)
        pa.res_mode, pa.res_relu, pa.sum_scale, pa.coeff, pa.scale_res = L.RES_ELTWISE, True, 1.0, (c, c), s_res
        ca = S.SaberConv2D(int8=True).init((N, Cc, H, Wd), pa, O.U8, O.S8, s_in, s_mid)
        cb = S.SaberConv2D(int8=True).init((N, K1, H, Wd), S.ConvParam(w2, b2, 1, (0, 0), (1, 1), (1, 1), bool(relu2)), O.S8, odt2, s_sum, s_out)
        ops.append((c0, ca, cb))
        wants.append((want1, want2))
        cur_x, cur_res, idt = want2, want1, odt2
    return ops, wants


def _site(rng, N, H, Wd, nblk, with_tail, idt, bdt):
    """pair + blocks + (optional) tail: device ops and the oracle's tensors"""
    xh = _rand8(rng, (N, H, Wd, 512), idt)
    a, b, want_a, want_b = _pair(rng, N, H, Wd, idt, bdt, xh)
    ops, wants = _blocks_from(rng, want_b, want_a, bdt, nblk)
    tail_ops, want_t = None, None
    if with_tail:
        last_dt = O.U8 if (nblk - 1) % 2 == 0 else O.S8
        c3t, cat, want_t = TT._head(rng, N, H, Wd, last_dt, O.U8, 1, x_in=wants[-1][1], res_in=wants[-1][0])
        tail_ops = (c3t, cat)
    return xh, (a, b), (want_a, want_b), ops, wants, tail_ops, want_t


HEAD_CASES = [
    # N, H, W, blocks, tail
    (2, 7, 9, 2, False),       # ragged, the last tile row half empty
    (1, 6, 16, 2, True),       # full width
    (3, 14, 14, 3, True),      # fewer images than XCDs
    (8, 14, 14, 5, True),      # res4 itself
]
# the head's input dtype, branch2a's output dtype (u8: with relu, s8: without)
VARIANTS = [(O.S8, O.U8), (O.U8, O.S8)]


@pytest.mark.parametrize("variant", VARIANTS, ids=["in_s8-b_relu_u8", "in_u8-b_s8"])
@pytest.mark.parametrize("case", HEAD_CASES)
def test_stage_with_head_equals_the_operators_and_oracle(case, variant):
    N, H, Wd, nblk, with_tail = case
    idt, bdt = variant
    rng = np.random.default_rng(9100 + N + H + nblk + idt)
    xh, (a, b), (want_a, want_b), ops, wants, tail_ops, want_t = _site(rng, N, H, Wd, nblk, with_tail, idt, bdt)
    chains = [S.SaberConvChain(ca, cb, conv3x3=c0) for c0, ca, cb in ops]
    y1 = [ca.new_output() for _, ca, _ in ops]
    y2 = [cb.new_output() for _, _, cb in ops]
    # the operators one by one
    dxh = dev(xh)
    ya, yb = a.new_output(), b.new_output()
    a.dispatch(dxh, ya)
    b.dispatch(dxh, yb)
    assert np.array_equal(host(ya), want_a) and np.array_equal(host(yb), want_b), "the pair's operators"
    cx, cr = yb, ya
    for k, (c0, ca, cb) in enumerate(ops):
        t0 = c0.new_output()
        c0.dispatch(cx, t0)
        ca.dispatch(t0, y1[k], cr)
        cb.dispatch(y1[k], y2[k])
        assert np.array_equal(host(y1[k]), wants[k][0]) and np.array_equal(host(y2[k]), wants[k][1]), ("operators", k)
        cx, cr = y2[k], y1[k]
    tail, yt = None, None
    if with_tail:
        c3t, cat = tail_ops
        t0, yt = c3t.new_output(), cat.new_output()
        c3t.dispatch(y2[-1], t0)
        cat.dispatch(t0, yt, y1[-1])
        assert np.array_equal(host(yt), want_t), "the tail's operators"
        tail = S.SaberConvChain(cat, None, conv3x3=c3t)
    # one launch, three times (the counters run on)
    stage = S.SaberChainStage(chains, tail=tail, head=(a, b))
    outs = y1 + y2 + [yb] + ([yt] if with_tail else [])
    for rep in range(3):
        for t in outs + [ya]:
            t.fill_(77)
        stage.dispatch_head(dxh, yb, y1, y2, yt)
        for k in range(nblk):
            assert np.array_equal(host(y1[k]), wants[k][0]), ("stage y1", k, rep)
            assert np.array_equal(host(y2[k]), wants[k][1]), ("stage y2", k, rep)
        assert np.array_equal(host(yb), want_b), ("head branch2a", rep)
        if with_tail:
            assert np.array_equal(host(yt), want_t), ("tail", rep)
    # the same stage object without its head: today's entry path, the same bits; the head's output tensor untouched
    for t in outs:
        t.fill_(77)
    if with_tail:
        stage.dispatch(dev(want_b), dev(want_a), y1, y2, yt)
        assert np.array_equal(host(yt), want_t)
    else:
        stage.dispatch(dev(want_b), dev(want_a), y1, y2)
    for k in range(nblk):
        assert np.array_equal(host(y1[k]), wants[k][0]) and np.array_equal(host(y2[k]), wants[k][1]), ("without the head", k)
    assert (host(yb) == 77).all()
    # ... and with it once more
    stage.dispatch_head(dxh, yb, y1, y2, yt)
    assert np.array_equal(host(y1[-1]), wants[-1][0]) and np.array_equal(host(y2[-1]), wants[-1][1]) and np.array_equal(host(yb), want_b)


def test_stage_refuses_a_head_it_cannot_run():
    """every refusal comes from where the stage is created, with its own message; the operators and chains of each case are built outside
    the `raises` block. (The seventh message, "stage: a head needs an image per XCD", guards the internal one-block form that spreads its
    tiles over all XCDs: the public entry points always create a stage with an image per XCD, so no caller can reach it.)"""
    rng = np.random.default_rng(12)
    N, H, Wd = 2, 6, 10

    def blocks(Cc=256, idt=O.U8):
        x = _rand8(rng, (N, H, Wd, Cc), idt)
        res = _rand8(rng, (N, H, Wd, 4 * Cc), O.S8)
        ops, _ = _blocks_from(rng, x, res, idt, 2, Cc=Cc)
        return [S.SaberConvChain(ca, cb, conv3x3=c0) for c0, ca, cb in ops], ops

    chains, keep = blocks()
    a, b, _, _ = _pair(rng, N, H, Wd, O.S8, O.U8)
    S.SaberChainStage(chains, head=(a, b))                                                     # (what the refusals below differ from)
    a256, _ = _conv1x1(rng, N, H, Wd, 256, 1024, O.S8, O.S8, False, 0.03, 0.04)                # C_in != 512
    b256, _ = _conv1x1(rng, N, H, Wd, 256, 256, O.S8, O.U8, True, 0.03, 0.02)
    with pytest.raises(L.SaberHipError, match="stage: the head's convs read 512 channels"):
        S.SaberChainStage(chains, head=(a256, b256))
    b3, _ = _conv1x1(rng, N, H, Wd, 512, 256, O.S8, O.U8, True, 0.03, 0.02, k=3, pad=1)        # a 3x3 / pad 1 conv
    with pytest.raises(L.SaberHipError, match="stage: the head must be two plain 1x1 / stride 1 / pad 0"):
        S.SaberChainStage(chains, head=(a, b3))
    a512, _ = _conv1x1(rng, N, H, Wd, 512, 512, O.S8, O.S8, False, 0.03, 0.04)                 # 512 output channels for the shortcut
    with pytest.raises(L.SaberHipError, match="stage: the head's convs write 1024 and 256 channels"):
        S.SaberChainStage(chains, head=(a512, b))
    bs8, _ = _conv1x1(rng, N, H, Wd, 512, 256, O.S8, O.S8, False, 0.03, 0.02)                  # block 0's 3x3 conv reads u8, this writes s8
    with pytest.raises(L.SaberHipError, match="stage: the head's outputs must be the first block's shortcut"):
        S.SaberChainStage(chains, head=(a, bs8))
    bh, _ = _conv1x1(rng, N, H + 2, Wd, 512, 256, O.S8, O.U8, True, 0.03, 0.02)                # another tensor shape
    with pytest.raises(L.SaberHipError, match="stage: the head's outputs must be the first block's shortcut"):
        S.SaberChainStage(chains, head=(a, bh))
    ar, _ = _conv1x1(rng, N, H, Wd, 512, 1024, O.S8, O.S8, False, 0.03, 0.04, res=True)        # a residual on the shortcut conv
    with pytest.raises(L.SaberHipError, match="stage: the head's convs carry no residual"):
        S.SaberChainStage(chains, head=(ar, b))
    chains128, keep128 = blocks(Cc=128)                                                        # a C = 128 stage
    with pytest.raises(L.SaberHipError, match="stage: a head goes with a C = 256 stage only"):
        S.SaberChainStage(chains128, head=(a, b))


# ------------------------------------------------------------------------------------------------ net level
@pytest.mark.parametrize("batch,hw", [(3, 96), (8, 224)])
def test_resnet50_net_runs_the_res4a_pair_as_the_stage_head(batch, hw):
    model, scales, x, ref = TT._resnet50(batch, hw)
    net = W.build_int8_net(model, dict(scales), batch, hw=hw, stage=True)
    net.tensor("data").copy_(torch.from_numpy(x).cuda())
    net.run()
    # the site is formed, the head is OFF after build and stays off when the stages go on: names and counts as without this form
    assert net.heads() == []
    assert not any("[pair1x1]" in net.op_name(i) for i in range(net.num_ops()))
    net.select_stages(True)
    stages = net.stages()
    res4 = [s for s in stages if net.op_name(s[0]).startswith("conv:stage_c256")]
    assert len(res4) == 1 and res4[0][1] == 5, stages
    i0, nb = res4[0][0], res4[0][1]
    ip = int(L.load().saber_hip_net_stage_head(net.h, i0))
    assert ip == i0 - 1 and [int(L.load().saber_hip_net_stage_head(net.h, s[0])) for s in stages if s[0] != i0] == [-1] * (len(stages) - 1)
    assert net.heads() == [] and "(in the" not in net.op_name(ip) and not net.unwritten("res4a_branch1")
    tails_off = net.tails()
    off = net.num_launches()
    names_off = [net.op_name(i) for i in range(net.num_ops())]
    ch_off = net.choices()
    _check = TT._check_edges
    # head on: one launch fewer, the shortcut edge stays in LDS
    net.select_heads(True)
    assert net.heads() == [(ip, i0)] and net.stages() == stages
    assert net.num_launches() == off - 1
    names_on = [net.op_name(i) for i in range(net.num_ops())]
    assert names_on[ip] == "conv:(in the stage launch)" and names_on[i0].startswith("conv:[pair1x1]+stage_c256"), (names_on[ip], names_on[i0])
    assert [n for i, n in enumerate(names_on) if i not in (ip, i0)] == [n for i, n in enumerate(names_off) if i not in (ip, i0)]
    assert net.unwritten("res4a_branch1") and not net.unwritten("res4a_branch2a")
    _check(net, x, ref, "head on")
    ch_on = net.choices()
    assert len(ch_on) == net.num_ops()
    # head off again: the edge is written and equal
    net.select_heads(False)
    assert net.heads() == [] and net.num_launches() == off and not net.unwritten("res4a_branch1")
    assert [net.op_name(i) for i in range(net.num_ops())] == names_off and net.choices() == ch_off
    _check(net, x, ref, "head off")
    # a stage switched off takes its head with it; switched on again it comes back without
    net.select_heads(True)
    net.select_stages(False)
    assert net.heads() == [] and "(in the" not in net.op_name(ip) and not net.unwritten("res4a_branch1")
    net.select_stages(True)
    net.select_tails(bool(tails_off))                           # (a stage word recorded while the stage was off carries no tail bit)
    assert net.heads() == [] and net.num_launches() == off
    assert [net.op_name(i) for i in range(net.num_ops())] == names_off
    if hw == 224:
        return
    # the decision travels through choices() / set_choices() to a fresh net, both ways
    fresh = W.build_int8_net(model, dict(scales), batch, hw=hw, stage=True)
    fresh.set_choices(ch_on)
    assert fresh.choices() == ch_on and fresh.heads() == [(ip, i0)] and fresh.num_launches() == off - 1
    assert [fresh.op_name(i) for i in range(fresh.num_ops())] == names_on
    fresh.set_choices(ch_off)
    assert fresh.choices() == ch_off and fresh.heads() == [] and fresh.num_launches() == off
    assert [fresh.op_name(i) for i in range(fresh.num_ops())] == names_off
    # a stage launch that did not complete: stage, tail and head fall back together, the next pass is right
    ch = list(ch_on)
    for i, _, _ in stages:
        if i != i0:
            ch[i] &= ~(1 << 30)                                 # res4 is the net's only selected stage
    net.set_choices(ch)
    head = (i0 + 3 * nb, i0 + 3 * nb + 1)
    ch = net.choices()
    ch[head[0]] &= ~(15 << 24)                                  # (the strided head's own form: two separate launches)
    net.set_choices(ch)
    net.select_tails(True)
    assert [s[0] for s in net.stages() if s[2]] == [i0] and net.tails() == [(i0, nb)] and net.heads() == [(ip, i0)]
    before = net.num_launches()
    L.check(L.load().saber_hip_net_inject_coop_error(net.h))
    with pytest.raises(L.SaberHipError):
        net.status()
    assert not any(s[2] for s in net.stages()) and net.tails() == [] and net.heads() == []
    assert net.num_launches() == before + nb - 1 + 2 + 1
    assert all("(in the" not in net.op_name(i) for i in head + (ip,))
    net.tensor("data").copy_(torch.from_numpy(x).cuda())
    net.run()
    net.status()
    assert np.array_equal(host(net.tensor("fc1000")), ref["fc1000"].reshape(host(net.tensor("fc1000")).shape))


# ------------------------------------------------------------------------------------------------ guard bands
def test_stage_with_head_between_guard_bands():
    """the smallest ragged case, every tensor of the launch between guard bands of both patterns (tests/guard_util.py): no guard byte
    changes, the outputs do not depend on the pattern and are the oracle's; the shortcut tensor is not part of the launch"""
    N, H, Wd, nblk, with_tail = HEAD_CASES[0]
    rng = np.random.default_rng(9177)
    xh, (a, b), (want_a, want_b), ops, wants, _, _ = _site(rng, N, H, Wd, nblk, with_tail, O.S8, O.U8)
    chains = [S.SaberConvChain(ca, cb, conv3x3=c0) for c0, ca, cb in ops]
    stage = S.SaberChainStage(chains, head=(a, b))
    outs = {"yb": (want_b.shape, want_b.dtype, None)}
    for k in range(nblk):
        outs["y1_%d" % k] = (wants[k][0].shape, wants[k][0].dtype, None)
        outs["y2_%d" % k] = (wants[k][1].shape, wants[k][1].dtype, None)

    def launch(T, ws):
        stage.dispatch_head(T["xh"], T["yb"], [T["y1_%d" % k] for k in range(nblk)], [T["y2_%d" % k] for k in range(nblk)])
    got = GU.run_guarded({"xh": xh}, outs, launch, "cuda", 0, plain=None, what="stage with head")
    torch.cuda.synchronize()
    want = {"yb": want_b}
    for k in range(nblk):
        want["y1_%d" % k], want["y2_%d" % k] = wants[k]
    for n, w in want.items():
        assert np.array_equal(got[n], w), n
        GU.assert_no_sentinel_run(got[n], "stage with head, output '%s'" % n)
