"""The conditions tests/test_gpu_live_weights.py rests on, proved without a device: for every case the oracle's output under the second
parameter set differs from the first set's and from every stale model's (tests/live_weights_util.py) in at least a quarter of the output
bytes - so an op that kept ONE ingredient of its first set_weights cannot pass the device test by chance -, the numpy model that computes
the stale outputs equals the oracle on both whole sets, and for every composite launch the combination include/saber_hip.h documents is told
from every other old / new combination of its members' parameters."""
import numpy as np
import pytest

from tests import live_weights_util as U


@pytest.mark.parametrize("geometry", U.GEOMETRY_NAMES)
def test_single_op_cases_tell_every_stale_model(geometry):
    lo = 1.0
    for name in U.case_names([geometry]):
        c = U.case(name)
        for which in "AB":
            assert np.array_equal(c.model_of(which), c.want[which]), (name, which, "the numpy model differs from the oracle")
        shares = {"A": U.share(c.want["B"], c.want["A"])}
        for kind in U.stale_kinds(c.spec):
            shares[kind] = U.share(c.want["B"], c.stale(kind))
        if c.spec.mode == "elt":      # the reverse mix is what a run with A's packing and B's scale gives: it must be told from want(A) too
            shares["reverse vs A"] = U.share(c.want["A"], c.stale("reverse"))
        print(name, " ".join("%s %.2f" % kv for kv in shares.items()))
        assert min(shares.values()) >= U.MIN_SHARE, (name, shares)
        lo = min(lo, min(shares.values()))
    print("%s: smallest share %.2f" % (geometry, lo))


@pytest.mark.parametrize("shape", U.FC_SHAPES)
@pytest.mark.parametrize("kind", U.FC_INPUTS)
def test_fc_cases_tell_every_stale_model(shape, kind):
    c = U.fc_case(shape, kind)
    shares = {"A": U.share(c.want["B"], c.want["A"])}
    for k in c.stale_kinds():
        shares[k] = U.share(c.want["B"], c.stale(k))
    print(shape, kind, " ".join("%s %.2f" % kv for kv in shares.items()))
    assert min(shares.values()) >= U.MIN_SHARE, (shape, kind, shares)


@pytest.mark.parametrize("shape", U.FC_SHAPES)
def test_fc_f32_cases_differ_by_far_more_than_the_tolerance(shape):
    from oracle import oracle as O
    x, sets = U.fc_f32_case(shape)
    a, b = O.fc_f32(x, *sets[0]), O.fc_f32(x, *sets[1])
    far = np.abs(a - b) > 100 * 1e-4 * np.abs(b).max()          # 100 x the FP32 tolerance of the device test
    assert far.mean() >= U.MIN_SHARE, (shape, far.mean())
    assert (np.abs(O.fc_f32(x, sets[1][0], None) - b) > 100 * 1e-4 * np.abs(b).max()).mean() >= U.MIN_SHARE      # bias -> None


@pytest.mark.parametrize("name", U.COMPOSITE_NAMES)
def test_composites_tell_the_documented_combination_from_every_other(name):
    comp = U.composite(name)
    for updated in comp.updates():
        doc = comp.documented(updated)
        want = comp.eval(doc)
        for pick in comp.other_picks(doc):
            got = comp.eval(pick)
            first = next(m for m in comp.names if pick[m] != doc[m])          # (its inputs are still the documented ones)
            assert not np.array_equal(got[first], want[first]), (name, sorted(updated), pick, first)
            # ... and on the tensors the launch WRITES (a chain's 3x3 edge stays in LDS): some written output tells the two apart
            assert any(not np.array_equal(got[m], want[m]) for m in comp.written), (name, sorted(updated), pick)
    a, b = comp.eval(comp.all("A")), comp.eval(comp.all("B"))
    shares = {m: U.share(a[m], b[m]) for m in comp.names}
    print(name, "live:", sorted(comp.live), " ".join("%s %.2f" % kv for kv in shares.items()))
    assert min(shares.values()) >= U.MIN_SHARE, (name, shares)
    for m in comp.names:          # no output sits on its rails: a saturated tensor would hide what fed it
        y = a[m]
        rails = np.mean((y == np.iinfo(y.dtype).max) | ((y == np.iinfo(y.dtype).min) & (y.dtype == np.int8)))
        assert rails < 0.6, (name, m, rails)
