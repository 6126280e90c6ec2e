"""tests/oplist_util.py without a GPU: the interpreter against the existing oracle walks, every perturbation changing exactly one thing, and -
what makes a pass of tests/test_gpu_net_legality.py mean something - every perturbed case DISCRIMINATING: the answer of the list with the
rewrite applied anyway (a removed edge reads as POISON, a moved write happens at the earlier position) differs from the right answer in at
least a quarter of the bytes of one of the tensors the GPU test compares. The share is a property of the inputs and scales (every edge's
own MAXABS scale: bytes between the rails), asserted here from the oracle alone."""
import numpy as np
import pytest

from oracle import net_oracle as NO
from oracle import oracle as O
from tests import oplist_util as U

ALL = sorted(U.PATTERNS)

# Cases the forced model cannot tell from the right answer, each with its reason. The CPU test asserts that they are exactly these.
#   lane:*          an op on the side lane changes no value: what a wrong rewrite risks is a cross-lane race, which has no deterministic answer
#   f1 in_place:b   conv + eltwise as one step that writes the (external) residual's tensor computes the bytes the two ops compute: element i
#   chain  "        of the output depends on element i of the residual only. The optimiser declines all the same (the fused kernel's
#   ir     "        residual read and its store are not ordered across workgroups' tiles by anything the executor promises)
INDISTINCT = {("f1", "in_place:b"), ("chain", "in_place:b"), ("ir", "in_place:b")}


def _indistinct(name, case):
    return case.startswith("lane:") or (name, case) in INDISTINCT


def _cases():
    return [(name, case) for name in ALL for case in U.perturbations(name)]


# ---- the interpreter against the existing oracles ------------------------------------------------------------------------------------------
def _bottleneck_model(rng, c=64, mid=32, hw=9):
    """one ResNet bottleneck over `data`: branch1 (1x1) and branch2a / 2b / 2c, the sum with relu - as workloads' spec entries"""
    spec = [{"kind": "conv", "name": "b1", "src": "data", "k": 1, "stride": 1, "pad": 0, "cout": c, "relu": False},
            {"kind": "conv", "name": "b2a", "src": "data", "k": 1, "stride": 1, "pad": 0, "cout": mid, "relu": True},
            {"kind": "conv", "name": "b2b", "src": "b2a", "k": 3, "stride": 1, "pad": 1, "cout": mid, "relu": True},
            {"kind": "conv", "name": "b2c", "src": "b2b", "k": 1, "stride": 1, "pad": 0, "cout": c, "relu": False},
            {"kind": "eltwise", "name": "res", "a": "b2c", "b": "b1", "relu": True},
            {"kind": "pool", "name": "pool", "src": "res", "win": 3, "stride": 2, "pad": 0, "type": 0}]
    cin = {"b1": c, "b2a": c, "b2b": mid, "b2c": mid}
    params = {l["name"]: ((rng.standard_normal((l["cout"], cin[l["name"]], l["k"], l["k"])) * np.sqrt(2.0 / (cin[l["name"]] * l["k"] ** 2))).astype(np.float32),
                          (rng.standard_normal(l["cout"]) * 0.3).astype(np.float32)) for l in spec if l["kind"] == "conv"}
    scales = {"data": 0.02, "b1": 0.05, "b2a": 0.03, "b2b": 0.04, "b2c": 0.06, "res": 0.07}
    return {"spec": spec, "params": params}, scales, rng.standard_normal((2, c, hw, hw)).astype(np.float32)


def test_interpreter_equals_the_net_oracle_on_a_bottleneck():
    rng = np.random.default_rng(41)
    model, scales, x = _bottleneck_model(rng)
    ref = NO.run_int8(model, dict(scales), x)
    d = U.Desc()
    xq = O.quant_nchw_to_nhwc(x, scales["data"], U.S8)      # (both convs over `data` quantise it on entry, with the same scale)
    d.tensors["data"] = (xq.shape, U.S8)
    d.inputs.append("data")
    for l in model["spec"]:
        nm = l["name"]
        d.tensors[nm] = (ref[nm].shape, O.code_of(ref[nm]))
        if l["kind"] == "conv":
            w, b = model["params"][nm]
            d.ops.append({"kind": "conv", "id": nm, "pat": None, "lane": 0, "in": l["src"], "out": nm, "w": w, "b": b, "s_in": scales[l["src"]],
                          "s_out": scales[nm], "relu": l["relu"], "pad": l["pad"], "stride": l["stride"], "group": 1})
        elif l["kind"] == "eltwise":
            c = float(np.float32(1.0 / scales[nm]))
            d.ops.append({"kind": "elt", "id": nm, "pat": None, "lane": 0, "a": l["a"], "b": l["b"], "out": nm, "sa": scales[l["a"]], "sb": scales[l["b"]],
                          "c0": c, "c1": c, "relu": l["relu"]})
        else:
            d.ops.append({"kind": "pool", "id": nm, "pat": None, "lane": 0, "in": l["src"], "out": nm, "win": l["win"], "stride": l["stride"],
                          "pad": l["pad"], "type": l["type"], "floor": False, "global": False})
    got, seen = U.run_oracle(d, {"data": xq})
    assert not seen
    for l in model["spec"]:
        assert np.array_equal(got[l["name"]], ref[l["name"]]), l["name"]
    assert U.outputs(d) == ["pool"] and U.required(d) == [l["name"] for l in model["spec"]]      # (no patterns: every reader is an outsider)


def test_interpreter_equals_the_branchy_nets_reference():
    d, x, coeffs = U.branchy_desc()
    got, _ = U.run_oracle(d, {"x": x})
    ref = {nm: O.eltwise_i8(x, x, 1.0, 1.0, np.float32(v), np.float32(v), False) for nm, v in coeffs.items()}
    ref["cat"] = np.concatenate([ref["a"], ref["b"], ref["c"]], -1)
    ref["out"] = O.eltwise_i8(ref["cat"], ref["cat"], 1.0, 1.0, np.float32(0.5), np.float32(0.5), True)
    ref["out2"] = O.eltwise_i8(ref["out"], ref["out"], 1.0, 1.0, np.float32(1.0), np.float32(0.5), False)
    for nm in ref:
        assert np.array_equal(got[nm], ref[nm]), nm


def test_overwrites_and_in_place_ops_follow_list_order():
    """a name written twice: every reader sees the value of its position, the final contents are the last write's; an in-place eltwise"""
    rng = np.random.default_rng(3)
    x, y = (rng.integers(-128, 128, (1, 2, 3, 16)).astype(np.int8) for _ in range(2))
    d = U.Desc()
    for nm in ("x", "y", "t", "r1", "r2"):
        d.tensors[nm] = ((1, 2, 3, 16), U.S8)
    d.inputs += ["x", "y"]
    elt = {"kind": "elt", "pat": None, "lane": 0, "sa": 0.1, "sb": 0.1, "c0": 4.0, "c1": 4.0, "relu": False}
    pool = {"kind": "pool", "pat": None, "lane": 0, "win": 1, "stride": 1, "pad": 0, "type": 0, "floor": False, "global": False}
    d.ops = [dict(elt, id="w1", a="x", b="y", out="t"), dict(pool, id="p1", out="r1", **{"in": "t"}), dict(elt, id="w2", a="t", b="x", out="t"),
             dict(pool, id="p2", out="r2", **{"in": "t"})]
    got, seen = U.run_oracle(d, {"x": x, "y": y})
    t1 = O.eltwise_i8(x, y, 0.1, 0.1, np.float32(4.0), np.float32(4.0), False)
    t2 = O.eltwise_i8(t1, x, 0.1, 0.1, np.float32(4.0), np.float32(4.0), False)
    assert not np.array_equal(t1, t2)
    assert np.array_equal(got["r1"], t1) and np.array_equal(got["t"], t2) and np.array_equal(got["r2"], t2)
    assert np.array_equal(seen[("p1", "t")], t1) and np.array_equal(seen[("w2", "t")], t1) and np.array_equal(seen[("p2", "t")], t2)
    assert sorted(U.outputs(d)) == ["r1", "r2"]


# ---- the patterns ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL + ["irsep", "irchain"])
def test_pattern_edges_lie_between_the_rails(name):
    """every 8-bit edge a pattern writes has at least a quarter of its bytes strictly between the rails (a relu leaves about half of an
    edge at zero; the scales are the edges' own MAXABS scales) - the condition under which a changed input changes the bytes"""
    desc, inputs, pat = U.pattern(name)
    vals, _ = U.run_oracle(desc, inputs)
    for nm in U.written(desc):
        v, dt = vals[nm], desc.tensors[nm][1]
        if dt == U.F32:
            assert np.isfinite(v).all(), nm
            continue
        lo, hi = (0, 255) if dt == U.U8 else (-128, 127)
        assert float(((v > lo) & (v < hi)).mean()) >= 0.25, (name, nm, float(((v > lo) & (v < hi)).mean()), int(v.min()), int(v.max()))
    assert set(pat.inner) <= set(U.written(desc)) and pat.out in U.outputs(desc)
    assert U.required(desc) == U.outputs(desc) or name in ("f2", "f512", "chain", "stage", "head")      # (patterns with two outputs read by nobody)


@pytest.mark.parametrize("name", ALL)
def test_every_perturbation_changes_exactly_one_thing(name):
    desc, inputs, pat = U.pattern(name)
    cases = U.perturbations(name)
    assert cases
    for case, (d, inp) in cases.items():
        added, removed, changed, moved = U.diff(desc, d)
        kind = case.split(":")[0]
        assert not removed and not moved, (name, case)
        if kind == "reader":
            assert added == ["xr"] and not changed and case.split(":")[1] in U.op_inputs(d.op("xr")), (name, case)
        elif kind == "rewrite_before_use":
            assert sorted(added) == ["rw_r", "rw_w"] and not changed and d.index("rw_w") < d.index(pat.moved[1]) < d.index("rw_r") < d.index(pat.moved[2])
            assert d.op("rw_w")["out"] == pat.moved[0] == d.op("rw_r")["in"]
        elif kind == "rewrite_source":
            assert added == ["rs_w"] and not changed and d.index(pat.source[1]) < d.index("rs_w") < d.index(pat.source[2]) and d.op("rs_w")["out"] == pat.source[0]
        elif kind == "in_place":
            assert not added and changed == [(pat.elt, "out")] and d.op(pat.elt)["out"] == d.op(pat.elt)[case[-1]]
        elif kind == "residual_late":
            assert added == ["late"] and not changed and d.index(pat.conv) < d.index("late") < d.index(pat.elt) and d.op("late")["out"] == pat.late
        elif kind == "lane":
            assert not added and changed == [(case.split(":")[1], "lane")]
        else:
            raise AssertionError(case)
        # the perturbed list is still a valid one: every input it names has a value of its shape and the oracle walks it
        U.run_oracle(d, inp)


_shares = {}


@pytest.mark.parametrize("name,case", _cases(), ids=["%s-%s" % nc for nc in _cases()])
def test_every_perturbed_case_is_discriminating(name, case):
    desc, inputs, pat = U.pattern(name)
    d, inp = U.perturbations(name)[case]
    share, where = U.share_changed(d, inp, pat)
    _shares[(name, case)] = share
    print("%s %s: the rewrite applied anyway changes %.3f of %s" % (name, case, share, where))
    if _indistinct(name, case):
        assert share == 0.0, (name, case, share, where)
    else:
        assert share >= 0.25, (name, case, share, where)


def test_the_unperturbed_patterns_are_what_the_forced_model_leaves_alone():
    """the control: with nothing perturbed, applying the rewrite changes no byte of any tensor the GPU test compares"""
    for name in ALL:
        desc, inputs, pat = U.pattern(name)
        share, where = U.share_changed(desc, inputs, pat)
        assert share == 0.0, (name, share, where)


def test_smallest_share():
    """the smallest share over every case the forced model can tell apart (computed here, whatever ran before)"""
    found = {}
    for name, case in _cases():
        if not _indistinct(name, case):
            d, inp = U.perturbations(name)[case]
            found[(name, case)] = _shares.get((name, case)) or U.share_changed(d, inp, U.pattern(name)[2])[0]
    k = min(found, key=found.get)
    print("smallest share over %d discriminating cases: %.3f (%s %s)" % (len(found), found[k], k[0], k[1]))
    assert len(found) >= 150 and found[k] >= 0.25
