"""tests/block_table.py without a GPU: every case tests/test_gpu_stage_blocks.py runs meets its preconditions in the oracle - no two
blocks share a record, a swapped or merged coefficient pair changes at least a quarter of a block's bytes, at least a tenth of them lie
between the rails, and under the saturating scales every edge holds bytes on each rail its dtype and relu leave it and unsaturated ones -
and a walk that applies block 0's record to every block gives other bytes in every later block."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import block_table as BT


@pytest.mark.parametrize("name", sorted(BT.CASES))
def test_case_meets_its_preconditions(name):
    run = BT.case(name)
    cond = run.conditions(name)
    assert len(cond) == (0 if run.sat else 2) and len(run.blocks) == 3
    assert [b.hand for b in run.blocks] == [O.U8, O.S8, O.U8] and [b.relu1 for b in run.blocks] == [0, 1, 0] and [b.res_relu for b in run.blocks] == [1, 0, 1]
    assert run.blocks[1].coeff[1] < 0 < run.blocks[1].coeff[0] and run.blocks[2].coeff[0] < run.blocks[2].coeff[1]
    print(name, [tuple(round(v, 3) for v in c) for c in cond])
    # block 0's record applied to a later block: its relu flags and coefficients on that block's own operands
    b0 = run.blocks[0]
    for k in (1, 2):
        b, e = run.blocks[k], run.edges[k]
        other = O.eltwise_i8(np.maximum(e["t1"][0], 0) if b0.relu1 else e["t1"][0], e["res"], b.s_mid, b.s_res, b0.coeff[0], b0.coeff[1], bool(b0.res_relu))
        assert (other != e["y1"][0]).mean() >= (0.05 if run.sat else 0.25), (name, k)


def test_rails_counts_what_the_dtype_and_relu_leave():
    y = np.array([-128, -5, 0, 127, 127], np.int8)
    assert BT.rails(y, O.S8, 0) == ([2, 1], 2) and BT.rails(y, O.S8, 1) == ([2], 2)
    assert BT.rails(np.array([0, 255, 9], np.uint8), O.U8, 0) == ([1], 1)


def test_coeff_conditions_refuses_a_pair_that_cannot_be_told_apart():
    rng = np.random.default_rng(3)
    a, r = BT.rand8(rng, (4, 64), O.S8), BT.rand8(rng, (4, 64), O.S8)
    BT.coeff_conditions(a, r, 0.05, 0.04, 20.0, -10.0, False, "ok")
    with pytest.raises(AssertionError):
        BT.coeff_conditions(a, r, 0.05, 0.04, 20.0, 20.0, False, "equal")
    with pytest.raises(AssertionError, match="between the rails"):
        BT.coeff_conditions(a, r, 0.05, 0.04, 2000.0, -1000.0, False, "all saturated")
