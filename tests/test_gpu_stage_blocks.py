"""Stage launches over blocks that DIFFER (tests/block_table.py): per block another hand-over dtype, relu on the first 1x1 conv, relu on the
sum and coefficient pair - (c, c), (c, -c / 2), (c / 2, c) - and other scales, through every stage form of conv_stage_coop.hip: C = 64, 128
and 256, C = 256 with the strided head as its tail (the tail's own pair unequal) and with the sibling pair as its head; once more per channel
count with every scale a quarter of its edge's MAXABS scale. The kernels read relu0 / relu1 / res_relu / relu2 / out_u8_2 / coeff_* from a
per-block record: a launch that applies block 0's record to every block, swaps the two coefficients, uses one for both or drops the sign
gives other bytes (asserted from the oracle before anything is launched). Every block's two outputs against the oracle walk, from the chain
launches and from three launches of one stage object."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from anakin_amd import lib as L  # noqa: E402
from anakin_amd import saber as S  # noqa: E402
from oracle import oracle as O  # noqa: E402
from tests import block_table as BT  # noqa: E402
from tests import test_gpu_stage_head as TH  # noqa: E402
from tests import test_gpu_stage_tail as TT  # noqa: E402

dev, host = TT.dev, TT.host


@pytest.fixture(scope="module", autouse=True)
def _device():
    L.require_device()


def _same(got, want, what):
    got = host(got)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        i = tuple(int(v) for v in bad[0])
        raise AssertionError("%s: %d of %d bytes differ from the oracle, first at %s: got %d, oracle %d" % (what, len(bad), want.size, i, int(got[i]), int(want[i])))


def _chains_then_stage(run, what):
    """the device operators of a run and its chain launches one by one, each against the oracle; returns (ops, chains, y1, y2)"""
    ops = BT.device_ops(run)
    chains = [S.SaberConvChain(ca, cb, conv3x3=c0) for c0, ca, cb in ops]
    y1 = [ca.new_output() for _, ca, _ in ops]
    y2 = [cb.new_output() for _, _, cb in ops]
    cx, cr = dev(run.x), dev(run.res)
    for k, ch in enumerate(chains):
        ch.dispatch(cx, cr, y1[k], y2[k])
        _same(y1[k], run.wants[k][0], "%s: chain %d y1 (%s)" % (what, k, ch.tile()))
        _same(y2[k], run.wants[k][1], "%s: chain %d y2 (%s)" % (what, k, ch.tile()))
        cx, cr = y2[k], y1[k]
    return ops, chains, y1, y2


@pytest.mark.parametrize("name", sorted(BT.CASES))
def test_stage_of_blocks_that_differ_equals_the_chains_and_oracle(name):
    run = BT.case(name)
    cond = run.conditions(name)
    print("%s: (swapped, conv's for both, between the rails) per block with an unequal pair: %s" % (name, [tuple(round(v, 3) for v in c) for c in cond]))
    ops, chains, y1, y2 = _chains_then_stage(run, name)
    stage = S.SaberChainStage(chains)
    xd, rd = dev(run.x), dev(run.res)
    for rep in range(3):                             # (the edge counters are never reset)
        for t in y1 + y2:
            t.fill_(77)
        stage.dispatch(xd, rd, y1, y2)
        for k in range(len(ops)):
            _same(y1[k], run.wants[k][0], "%s: stage block %d y1, launch %d" % (name, k, rep))
            _same(y2[k], run.wants[k][1], "%s: stage block %d y2, launch %d" % (name, k, rep))
    if run.c == 64:                                  # the form that leaves the inner blocks' first outputs unwritten
        for t in y1 + y2:
            t.fill_(77)
        stage.dispatch(xd, rd, [None] * (len(ops) - 1) + [y1[-1]], y2)
        for k in range(len(ops)):
            _same(y2[k], run.wants[k][1], "%s: inner y1 skipped, block %d y2" % (name, k))
        _same(y1[-1], run.wants[-1][0], "%s: inner y1 skipped, the last y1" % name)
        assert all((host(t) == 77).all() for t in y1[:-1])


@pytest.mark.parametrize("pair", BT.UNEQUAL)
def test_stage_with_tail_of_blocks_that_differ(pair):
    """TT.TAIL_CASES[0]: two blocks of the table (u8 then s8 hand-over) and the strided head as the launch's tail, its own pair unequal"""
    N, H, Wd, nblk, mdt, res_relu = TT.TAIL_CASES[0]
    rng = np.random.default_rng(7400 + int(10 * pair[0]))
    run = BT.Run(rng, BT.rand8(rng, (N, H, Wd, 256), O.U8), BT.rand8(rng, (N, H, Wd, 1024), O.S8), O.U8, 256, BT.TABLE[:nblk])
    run.conditions("tail run")
    d = {}
    c3t, cat, want_t = TT._head(rng, N, H, Wd, run.last_dt, mdt, res_relu, x_in=run.wants[-1][1], res_in=run.wants[-1][0], coeff=pair, detail=d)
    print("tail %s: %s" % (pair, BT.coeff_conditions(d["t1"], d["res"], d["s0"], d["s1"], d["coeff"][0], d["coeff"][1], d["relu"], "tail", d["want"])))
    ops, chains, y1, y2 = _chains_then_stage(run, "tail run")
    tail = S.SaberConvChain(cat, None, conv3x3=c3t)
    yt = cat.new_output()
    tail.dispatch(y2[-1], y1[-1], yt)
    _same(yt, want_t, "the head's chain launch")
    stage = S.SaberChainStage(chains, tail=tail)
    for rep in range(3):
        for t in y1 + y2 + [yt]:
            t.fill_(77)
        stage.dispatch(dev(run.x), dev(run.res), y1, y2, yt)
        for k in range(nblk):
            _same(y1[k], run.wants[k][0], "stage + tail block %d y1, launch %d" % (k, rep))
            _same(y2[k], run.wants[k][1], "stage + tail block %d y2, launch %d" % (k, rep))
        _same(yt, want_t, "tail, launch %d" % rep)


def test_stage_with_head_of_blocks_that_differ():
    """tests/test_gpu_stage_head.py's smallest case (2 x 7 x 9, two blocks, s8 input, branch2a relu / u8): the sibling pair inside the
    launch, in front of two blocks of the table"""
    N, H, Wd, nblk, _ = TH.HEAD_CASES[0]
    idt, bdt = TH.VARIANTS[0]
    rng = np.random.default_rng(9200)
    xh = TH._rand8(rng, (N, H, Wd, 512), idt)
    a, b, want_a, want_b = TH._pair(rng, N, H, Wd, idt, bdt, xh)
    run = BT.Run(rng, want_b, want_a, bdt, 256, BT.TABLE[:nblk])
    run.conditions("head run")
    ops, chains, y1, y2 = _chains_then_stage(run, "head run")
    stage = S.SaberChainStage(chains, head=(a, b))
    yb = b.new_output()
    for rep in range(3):
        for t in y1 + y2 + [yb]:
            t.fill_(77)
        stage.dispatch_head(dev(xh), yb, y1, y2)
        _same(yb, want_b, "head branch2a, launch %d" % rep)
        for k in range(nblk):
            _same(y1[k], run.wants[k][0], "head + stage block %d y1, launch %d" % (k, rep))
            _same(y2[k], run.wants[k][1], "head + stage block %d y2, launch %d" % (k, rep))
