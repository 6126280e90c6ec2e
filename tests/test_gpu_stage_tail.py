"""The res4 stage launch with a TAIL (conv_stage_coop.hip, saber_hip_conv2d_stage_create_tail): behind its blocks the persistent launch runs
the strided head that follows the stage in ResNet - res4f's conv 3x3 / stride 2 and conv 1x1 + eltwise on the shortcut sub-sampled by 2 - on
the halo and the shortcut tile the last block left on the CU. Integer sums and the separate operators' float sequence: every tensor the
launch writes holds the bits of the operators dispatched one by one (= the oracle's), launch after launch (its counters are never reset),
for ragged images, both hand-over dtypes and both eltwise forms; what the kernel cannot run is refused when the stage is created; and at net
level (ResNet50's framework list) the tail form and the separate head write identical edges, eager and as a hipGraph, survive a
choices() round trip and fall back together with the stage."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from anakin_amd import lib as L  # noqa: E402
from anakin_amd import saber as S  # noqa: E402
from anakin_amd import workloads as W  # noqa: E402
from oracle import oracle as O  # noqa: E402
from oracle import net_oracle as NO  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _device():
    L.require_device()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _res4_blocks(rng, N, H, Wd, nblk, first_u8=True, Cc=256):
    """tests/test_gpu_parity.py's helper: nblk block chains [3x3 -> 1x1 expand + eltwise(relu) -> next block's 1x1 reduce], chain i + 1 reading
    chain i's outputs; the last conv's output dtype alternates u8 / s8 with the block index. Returns the device ops, the first inputs and the
    oracle's outputs per block."""
    K1 = 4 * Cc
    x = rng.integers(0, 256, (N, H, Wd, Cc)).astype(np.uint8) if first_u8 else rng.integers(-128, 128, (N, H, Wd, Cc)).astype(np.int8)
    res = rng.integers(-128, 128, (N, H, Wd, K1)).astype(np.int8)
    ops, wants = [], []
    cur_x, cur_res, idt = x, res, (O.U8 if first_u8 else O.S8)
    for k in range(nblk):
        w0 = (rng.standard_normal((Cc, Cc, 3, 3)) * np.sqrt(2.0 / (9 * Cc))).astype(np.float32)
        b0 = (rng.standard_normal(Cc) * 0.5).astype(np.float32)
        w1 = (rng.standard_normal((K1, Cc, 1, 1)) * np.sqrt(2.0 / Cc)).astype(np.float32)
        b1 = (rng.standard_normal(K1) * 0.5).astype(np.float32)
        w2 = (rng.standard_normal((Cc, K1, 1, 1)) * np.sqrt(2.0 / K1)).astype(np.float32)
        b2 = (rng.standard_normal(Cc) * 0.5).astype(np.float32)
        s_x, s_in, s_mid, s_res, s_sum, s_out = 0.023 + 0.001 * k, 0.02, 0.05, 0.043 + 0.002 * k, 0.06, 0.031
        c = 1.0 / s_sum
        odt2 = O.U8 if k % 2 == 0 else O.S8          # the next block's 3x3 input: both kinds
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
    return x, res, ops, wants


def _head(rng, N, H, Wd, idt, mdt, res_relu, Cc=256, stride=2, res_stride=2, x_in=None, res_in=None, res_hw=None, coeff=(1.0, 1.0), detail=None):
    """the strided head behind a run of blocks: conv 3x3 / stride `stride` / pad 1 (C -> C, reads dtype idt, writes mdt) and conv 1x1 (C -> 4C)
    + eltwise on the shortcut [N][H][Wd][4C] sub-sampled by res_stride. Returns the two device ops and - given the oracle's inputs - its output.
    coeff: the eltwise's pair as multiples of 1 / s_sum; detail: a dict that receives the eltwise's operands, scales and coefficients."""
    K1 = 4 * Cc
    Ho, Wo = (H + 2 - 3) // stride + 1, (Wd + 2 - 3) // stride + 1
    w0 = (rng.standard_normal((Cc, Cc, 3, 3)) * np.sqrt(2.0 / (9 * Cc))).astype(np.float32)
    b0 = (rng.standard_normal(Cc) * 0.5).astype(np.float32)
    w1 = (rng.standard_normal((K1, Cc, 1, 1)) * np.sqrt(2.0 / Cc)).astype(np.float32)
    b1 = (rng.standard_normal(K1) * 0.5).astype(np.float32)
    s_x, s_in, s_mid, s_res, s_sum = 0.031, 0.02, 0.05, 0.06, 0.07
    c = 1.0 / s_sum
    cc = (float(np.float32(coeff[0] * c)), float(np.float32(coeff[1] * c))) if tuple(coeff) != (1.0, 1.0) else (c, c)
    relu0 = mdt == O.U8
    c0 = S.SaberConv2D(int8=True).init((N, Cc, H, Wd), S.ConvParam(w0, b0, 1, (1, 1), (stride, stride), (1, 1), bool(relu0)), idt, mdt, s_x, s_in)
    pa = S.ConvParam(w1, b1, 1, (0, 0), (1, 1), (1, 1), False)
    pa.res_mode, pa.res_relu, pa.sum_scale, pa.coeff, pa.scale_res = L.RES_ELTWISE, bool(res_relu), 1.0, cc, s_res
    if res_stride > 1:
        pa.res_stride, pa.res_hw = res_stride, res_hw or (H, Wd)
    ca = S.SaberConv2D(int8=True).init((N, Cc, Ho, Wo), pa, mdt, O.S8, s_in, s_mid)
    want = None
    if x_in is not None:
        ws0 = O.weight_scales(w0)
        bp0, sc0 = O.conv_i8_prepare(ws0, b0, s_x, s_in, idt, mdt)
        t0 = O.conv_i8(x_in, O.quant_weights(w0, ws0), bp0, sc0, mdt, int(relu0), (1, 1), (stride, stride))
        ws1 = O.weight_scales(w1)
        bp1, sc1 = O.conv_i8_prepare(ws1, b1, s_in, s_mid, mdt, O.S8)
        t1 = O.conv_i8(t0, O.quant_weights(w1, ws1), bp1, sc1, O.S8, 0)
        sub = O.pool_i8_nhwc(res_in, (1, 1), (2, 2), (0, 0), 0, floor_mode=True)
        want = O.eltwise_i8(t1, sub, s_mid, s_res, cc[0], cc[1], bool(res_relu))
        if detail is not None:
            detail.update(t1=t1, res=sub, s0=s_mid, s1=s_res, coeff=cc, relu=bool(res_relu), want=want)
    return c0, ca, want


TAIL_CASES = [
    # N, H, W, blocks, dtype 3x3 -> 1x1 of the tail, relu after the tail's sum
    (2, 7, 9, 2, O.S8, 0),       # odd H and W: the last output row / column reads padding, W' = 5; an s8 hand-over (two blocks)
    (1, 6, 16, 2, O.U8, 1),      # full width, W' = 8
    (3, 14, 14, 3, O.U8, 0),     # a u8 hand-over (three blocks), fewer images than XCDs
    (8, 14, 14, 5, O.U8, 1),     # res4 of ResNet50 at batch 8
]


@pytest.mark.parametrize("case", TAIL_CASES)
def test_stage_with_tail_equals_the_operators_and_oracle(case):
    N, H, Wd, nblk, mdt, res_relu = case
    rng = np.random.default_rng(7300 + N + H + nblk)
    x, res, ops, wants = _res4_blocks(rng, N, H, Wd, nblk)
    last_dt = O.U8 if (nblk - 1) % 2 == 0 else O.S8
    c3t, cat, want_t = _head(rng, N, H, Wd, last_dt, mdt, res_relu, x_in=wants[-1][1], res_in=wants[-1][0])
    assert want_t.shape == (N, (H + 1) // 2, (Wd + 1) // 2, 1024)
    chains = [S.SaberConvChain(ca, cb, conv3x3=c0) for c0, ca, cb in ops]
    y1 = [ca.new_output() for _, ca, _ in ops]
    y2 = [cb.new_output() for _, _, cb in ops]
    # the operators one by one
    cx, cr = dev(x), dev(res)
    for k, (c0, ca, cb) in enumerate(ops):
        t0 = c0.new_output()
        c0.dispatch(cx, t0)
        ca.dispatch(t0, y1[k], cr)
        cb.dispatch(y1[k], y2[k])
        assert np.array_equal(host(y1[k]), wants[k][0]) and np.array_equal(host(y2[k]), wants[k][1]), ("operators", k)
        cx, cr = y2[k], y1[k]
    t0, yt = c3t.new_output(), cat.new_output()
    c3t.dispatch(y2[-1], t0)
    cat.dispatch(t0, yt, y1[-1])
    assert np.array_equal(host(yt), want_t), "the head's operators"
    # one launch
    tail = S.SaberConvChain(cat, None, conv3x3=c3t)
    stage = S.SaberChainStage(chains, tail=tail)
    for rep in range(3):
        for t in y1 + y2 + [yt]:
            t.fill_(77)
        stage.dispatch(dev(x), dev(res), y1, y2, yt)
        for k in range(nblk):
            assert np.array_equal(host(y1[k]), wants[k][0]), ("stage y1", k, rep)
            assert np.array_equal(host(y2[k]), wants[k][1]), ("stage y2", k, rep)
        assert np.array_equal(host(yt), want_t), ("tail", rep)
    # the same stage without its tail: the blocks only, the tail's output untouched
    for t in y1 + y2 + [yt]:
        t.fill_(77)
    stage.dispatch(dev(x), dev(res), y1, y2)
    assert np.array_equal(host(y1[-1]), wants[-1][0]) and np.array_equal(host(y2[-1]), wants[-1][1])
    assert (host(yt) == 77).all()


def test_stage_refuses_a_tail_it_cannot_run():
    """every refusal comes from where the stage (or, for a shortcut not sub-sampled by 2, the head's chain) is created, with its own message;
    the operators and chains of each case are built outside the `raises` block"""
    rng = np.random.default_rng(11)

    def blocks(N=2, H=6, Wd=10, nblk=2, Cc=256):
        _, _, ops, _ = _res4_blocks(rng, N, H, Wd, nblk, Cc=Cc)
        return [S.SaberConvChain(ca, cb, conv3x3=c0) for c0, ca, cb in ops], ops

    def head_chain(*a, **kw):
        c0, ca, _ = _head(rng, *a, **kw)
        return S.SaberConvChain(ca, None, conv3x3=c0), (c0, ca)

    chains, ops = blocks()
    good, keep = head_chain(2, 6, 10, O.S8, O.U8, 1)
    S.SaberChainStage(chains, tail=good)                                                      # (what the refusals below differ from)
    t, keep = head_chain(2, 6, 10, O.S8, O.U8, 1, stride=1, res_stride=0)                     # a stride-1 3x3 conv
    with pytest.raises(L.SaberHipError, match="stage: the tail must be a conv3x3 / stride 2"):
        S.SaberChainStage(chains, tail=t)
    t = S.SaberConvChain(ops[1][1], ops[1][2], conv3x3=ops[1][0])                             # a tail with a second 1x1 conv
    with pytest.raises(L.SaberHipError, match="stage: the tail must be a conv3x3 / stride 2"):
        S.SaberChainStage(chains, tail=t)
    # a shortcut sub-sampled by 4 (a valid operator: its shortcut is 9 x 17 for the 3 x 5 output): no chain takes it, so no stage can
    c0, ca, _ = _head(rng, 2, 6, 10, O.S8, O.U8, 1, res_stride=4, res_hw=(9, 17))
    with pytest.raises(L.SaberHipError, match="chain: a stride-2 head goes with a shortcut sub-sampled by 2"):
        S.SaberConvChain(ca, None, conv3x3=c0)
    t, keep = head_chain(2, 6, 10, O.U8, O.U8, 1)                                             # the tail reads u8, the last block writes s8
    with pytest.raises(L.SaberHipError, match="stage: the tail's 3x3 conv reads what the last block"):
        S.SaberChainStage(chains, tail=t)
    chains128, _ = blocks(Cc=128)                                                             # a C = 128 stage
    t, keep = head_chain(2, 6, 10, O.S8, O.U8, 1, Cc=128)
    with pytest.raises(L.SaberHipError, match="stage: a tail goes with a C = 256 stage only"):
        S.SaberChainStage(chains128, tail=t)
    one, _ = blocks(nblk=1)                                                                   # a one-block stage (its last conv writes u8)
    t, keep = head_chain(2, 6, 10, O.U8, O.U8, 1)
    with pytest.raises(L.SaberHipError, match="stage: a tail needs 2..23 blocks"):
        S.SaberChainStage(one, tail=t)
    nine, _ = blocks(N=9)                                                                     # batch 9: an image per XCD needs <= 8
    t, keep = head_chain(9, 6, 10, O.S8, O.U8, 1)
    with pytest.raises(L.SaberHipError, match="stage: an image per XCD needs batch <= 8"):
        S.SaberChainStage(nine, tail=t)


# ------------------------------------------------------------------------------------------------ net level
_MODEL = {}


def _resnet50(batch, hw):
    """model, scales, input and the oracle's edges: computed once per (batch, hw) and shared, never changed"""
    if (batch, hw) not in _MODEL:
        if "model" not in _MODEL:
            _MODEL["model"] = W.framework_model(W.build_model("resnet50"), "int8")
        model = _MODEL["model"]
        x = W.make_input(batch, hw=hw)
        scales = W.calibrate(model, x[:2])
        _MODEL[(batch, hw)] = (model, scales, x, NO.run_int8(model, dict(scales), x))
    return _MODEL[(batch, hw)]


def _check_edges(net, x, ref, what):
    for form in ("eager", "graph"):
        for nm in net.tensors:
            if nm != "data" and not net.unwritten(nm):
                net.tensor(nm).zero_()
        net.tensor("data").copy_(torch.from_numpy(x).cuda())
        if form == "eager":
            net.run()
        else:
            net.capture()
            net.replay()
        checked = 0
        for nm in net.tensors:
            if nm == "data" or nm not in ref or net.unwritten(nm):
                continue
            got, want = host(net.tensor(nm)), ref[nm]
            if nm == "prob":
                assert np.abs(got - want.reshape(got.shape)).max() <= 1e-4 * want.max()
            else:
                assert np.array_equal(got, want.reshape(got.shape)), (what, form, nm)
            checked += 1
        assert checked >= 40, checked


@pytest.mark.parametrize("batch,hw", [(8, 224), (3, 96)])
def test_resnet50_net_runs_res4f_as_the_stage_tail(batch, hw):
    model, scales, x, ref = _resnet50(batch, hw)
    net = W.build_int8_net(model, dict(scales), batch, hw=hw, stage=True)
    net.tensor("data").copy_(torch.from_numpy(x).cuda())
    net.run()
    net.select_stages(True)
    stages = net.stages()
    res4 = [s for s in stages if net.op_name(s[0]).startswith("conv:stage_c256")]
    assert len(res4) == 1 and res4[0][1] == 5, stages          # saber_hip_net_stage_blocks: the ordinary blocks
    i0, nb = res4[0][0], res4[0][1]
    head = (i0 + 3 * nb, i0 + 3 * nb + 1)
    # the head's own form pinned to two separate launches (chain code 0 on its 3x3 conv): the launch counts below are then about the tail alone
    ch = net.choices()
    ch[head[0]] &= ~(15 << 24)
    net.set_choices(ch)
    # tail on
    net.select_tails(True)
    assert net.tails() == [(i0, nb)]                            # the C = 128 stage has none and ignores the bit
    on = net.num_launches()
    names_on = [net.op_name(i) for i in range(net.num_ops())]
    assert all(names_on[i] == "conv:(in the stage launch)" for i in head), [names_on[i] for i in head]
    assert net.unwritten("res4f_branch2b")
    _check_edges(net, x, ref, "tail on")
    ch_on = net.choices()
    # tail off: the head's two launches come back, nothing else moves
    net.select_tails(False)
    assert net.tails() == [] and net.stages() == stages
    assert net.num_launches() == on + 2
    names_off = [net.op_name(i) for i in range(net.num_ops())]
    assert all("(in the" not in names_off[i] for i in head), [names_off[i] for i in head]
    assert not net.unwritten("res4f_branch2b")
    _check_edges(net, x, ref, "tail off")
    ch_off = net.choices()
    if hw == 224:
        return
    # the decision travels through choices() / set_choices() to a fresh net, both ways
    fresh = W.build_int8_net(model, dict(scales), batch, hw=hw, stage=True)
    fresh.set_choices(ch_on)
    assert fresh.choices() == ch_on and fresh.tails() == [(i0, nb)] and fresh.num_launches() == on
    assert [fresh.op_name(i) for i in range(fresh.num_ops())] == names_on
    fresh.set_choices(ch_off)
    assert fresh.choices() == ch_off and fresh.tails() == [] and fresh.num_launches() == on + 2
    assert [fresh.op_name(i) for i in range(fresh.num_ops())] == names_off
    # a stage launch that did not complete: stage and tail fall back together, the next pass is right
    ch = list(ch_on)
    for i, _, _ in stages:
        if i != i0:
            ch[i] &= ~(1 << 30)                                 # res4 is the net's only selected stage
    net.set_choices(ch)
    assert [s[0] for s in net.stages() if s[2]] == [i0] and net.tails() == [(i0, nb)]
    before = net.num_launches()
    L.check(L.load().saber_hip_net_inject_coop_error(net.h))
    with pytest.raises(L.SaberHipError):
        net.status()
    assert not any(s[2] for s in net.stages()) and net.tails() == []
    assert net.num_launches() == before + nb - 1 + 2
    assert all("(in the" not in net.op_name(i) for i in head)
    net.tensor("data").copy_(torch.from_numpy(x).cuda())
    net.run()
    net.status()
    assert np.array_equal(host(net.tensor("fc1000")), ref["fc1000"].reshape(host(net.tensor("fc1000")).shape))


def test_restored_choices_keep_the_blocks_of_a_selected_stage_inside_its_launch():
    """saber_hip_net_set_choice: choice words recorded while a stage was OFF carry, for every block but the first, whatever form the block's
    chain had then (at C = 256 by default not the 3x3-led one). Restored with the stage bit set, the stage head comes first and takes all its
    blocks' ops into its launch; the later words must not hand a block's followers back to a chain launch beside the stage."""
    batch, hw = 3, 96                      # (below batch 4 the optimiser leaves the stage off: the words are recorded in that state)
    model, scales, x, ref = _resnet50(batch, hw)
    net = W.build_int8_net(model, dict(scales), batch, hw=hw, stage=True)
    assert not any(s[2] for s in net.stages())
    off = net.num_launches()
    names_off = [net.op_name(i) for i in range(net.num_ops())]
    net.select_stages(True)
    net.select_tails(False)
    expected = off
    for i0, nb, on in net.stages():
        assert on
        inside = range(i0 + 1, i0 + 3 * nb)
        assert all("(in the" in net.op_name(i) for i in inside), [net.op_name(i) for i in inside]
        expected -= sum("(in the" not in names_off[i] for i in inside)
        for k in range(nb):
            assert "(in the" in net.op_name(i0 + 3 * k + 1) and "(in the" in net.op_name(i0 + 3 * k + 2)
    assert net.num_launches() == expected
    net.tensor("data").copy_(torch.from_numpy(x).cuda())
    net.run()
    assert np.array_equal(host(net.tensor("fc1000")), ref["fc1000"].reshape(host(net.tensor("fc1000")).shape))
