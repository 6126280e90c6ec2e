"""The DetectionOutput op on the GPU where detout.hip splits its work (tests/detout_util.py SCALE_CASES; tests/test_detout_cpu.py asserts
that each case reaches what it is named for): suppression across the 64-bit words of the mask form's matrix and a partly filled last word
(dense_k*), more kept boxes than the direct form's vote has lanes (kept_past_256), the chunked selection over ties, seams, sparse fills and
empty chunks (sel_*), more classes than the pack kernel has lanes and a per-image cut over more entries than one sort holds (cls_*, cut_ties_*),
batch 17 and the degenerate ends, and a random sweep of 48 descriptors. Both forms against the float32 restatement with test_gpu_detout's
check(): count, every column, the row order and the padding rows `==`, the forms `==` each other; eta < 1 has form 0 only."""
import numpy as np
import pytest

from tests import detout_util as DU
from tests import guard_util as GU
from tests import test_gpu_detout as T

pytestmark = pytest.mark.gpu
_REF = {}


def ref(name):
    """a scale case, its inputs and the restatement's (y, count), computed once"""
    if name not in _REF:
        cs = DU.scale_case(name)
        ins = DU.scale_inputs(name)
        y, c = DU.detout_ref(cs, *ins)
        y.setflags(write=False)
        c.setflags(write=False)
        _REF[name] = (cs, ins, (y, c))
    return _REF[name]


RUNS = [(name, form) for name in DU.scale_names() for form in ((0, 1) if DU.scale_case(name)["eta"] == 1.0 else (0,))]


@pytest.mark.parametrize("name,form", RUNS)
def test_scale_case_against_the_restatement(name, form):
    cs, ins, want = ref(name)
    op = T.make_op(cs)
    assert op.forms() == ([0] if cs["eta"] < 1 else [0, 1]) and op.out_rows() == cs["n"] * cs["keep"]
    got = T.run(op, *ins, form)
    T.check(got, want, name, cs["code"])
    if form == 1:      # the forms are bit-identical to each other
        other = T.run(op, *ins, 0)
        assert DU.same_bits(got[0], other[0]) and DU.same_bits(got[1], other[1])


@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("name", ["dense_k1024", "cls_300_cut"])
def test_scale_case_between_guard_bands(name, form):
    """sixteen mask words, the largest LDS request; a second block of classes under an active cut: no byte outside the tensors is touched"""
    cs, (loc, conf, prior), want = ref(name)
    op = T.make_op(cs)
    op.set_tile(form)

    def launch(t, ws):
        op.run(t["loc"], t["conf"], t["prior"], t["y"], t["count"])

    def plain(ins, outs, ws_bytes):
        t = {k: (None if v is None else T.dev(v)) for k, v in ins.items()}
        t["y"], t["count"] = op.new_outputs()
        return t, None
    got = GU.run_guarded({"loc": loc, "conf": conf, "prior": prior},
                         {"y": ((op.out_rows(), 7), np.float32, None), "count": ((1 + cs["n"],), np.int32, None)}, launch, plain=plain,
                         what="%s form %d" % (name, form))
    T.check((got["y"], got["count"]), want, name, cs["code"])


@pytest.mark.parametrize("form", [0, 1])
def test_second_run_keeps_far_fewer_boxes_in_dirty_buffers(form):
    """dense_k1024, then the same op, outputs and scratch with 40 candidates per class: no row, count or kept entry of the first run survives"""
    name = "dense_k1024"
    cs, (loc, conf, prior), want = ref(name)
    op = T.make_op(cs)
    y, count = op.new_outputs()
    y.fill_(float("nan"))
    first = T.run(op, loc, conf, prior, form, y, count)
    T.check(first, want, name)
    conf2 = conf.copy()
    conf2[:, :, 40:] = np.float32(-1.0)
    want2 = DU.detout_ref(cs, loc, conf2, prior)
    assert 0 < want2[1][0] < 80 < first[1][0]
    T.check(T.run(op, loc, conf2, prior, form, y, count), want2, "fewer rows into the same buffers")
    T.check(T.run(op, loc, conf, prior, form, y, count), want, "and the full case again")
