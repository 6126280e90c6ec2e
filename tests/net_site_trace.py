"""The scripted walk behind tests/test_gpu_net_sites.py: every way the op-list executor's launch SITES (1x1 chain, 3x3-led chain, strided head
+ pair, stage, stage tail, stage head, stem pair, separable pair) can be switched from outside - choice words one op at a time, the selectors,
whole choices() lists carried to a fresh net, a cooperative launch that reports a failure - and, after every step, a snapshot of everything
the executor derives from those decisions: the op names, the choice words, the launch count, the selected stages / tails / heads and which
edges are not written. tests/golden/net_site_trace.json holds the snapshots recorded once (scripts/record_net_site_trace.py) by the code as
it stood BEFORE the decisions and the derived state were separated (net_resolve); the code under test never regenerates it.

No autotuner runs inside the walk (its outcome depends on timing): with the static selection every name is deterministic.
Nothing here touches the GPU at import."""
import json
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "net_site_trace.json")
_SPARSE = ("names", "choices", "unwritten")      # per-op / per-tensor lists: the file stores the entries that changed since the step before


def snapshot(net, rc=0):
    from anakin_amd import lib as L
    lib = L.load()
    return {"rc": int(rc),
            "names": [net.op_name(i) for i in range(net.num_ops())],
            "choices": net.choices(),
            "launches": int(net.num_launches()),
            "stages": [list(s) for s in net.stages()],
            "tails": [list(s) for s in net.tails()],
            "heads": [list(s) for s in net.heads()],
            "unwritten": [int(lib.saber_hip_net_tensor_unwritten(net.h, t)) for t in range(net.num_tensors())]}


class Trace:
    """[(label, snapshot)] in walk order"""

    def __init__(self):
        self.steps = []

    def rec(self, label, net, rc=0):
        self.steps.append((label, snapshot(net, rc)))


def encode(steps):
    """[(label, snapshot)] -> a JSON-able list; every snapshot but the first as its difference from the one before"""
    out, prev = [], None
    for label, cur in steps:
        d = {}
        for k, v in cur.items():
            p = None if prev is None else prev[k]
            if p == v:
                continue
            if k in _SPARSE and p is not None and len(p) == len(v):
                d[k + "@"] = [[i, b] for i, (a, b) in enumerate(zip(p, v)) if a != b]
            else:
                d[k] = v
        out.append([label, d])
        prev = cur
    return out


def decode(enc):
    steps, prev = [], {}
    for label, d in enc:
        cur = {k: (list(v) if isinstance(v, list) else v) for k, v in prev.items()}
        for k, v in d.items():
            if k.endswith("@"):
                for i, b in v:
                    cur[k[:-1]][i] = b
            else:
                cur[k] = v
        steps.append((label, cur))
        prev = cur
    return steps


def load_golden():
    with open(GOLDEN) as f:
        return {k: decode(v) for k, v in json.load(f).items()}


# ------------------------------------------------------------------------------------------------------------------------------ helpers
def _set(net, i, word):
    """saber_hip_net_set_choice's status (a refused word changes nothing and is part of the trace)"""
    from anakin_amd import lib as L
    return int(L.load().saber_hip_net_set_choice(net.h, int(i), int(word)))


def _signed(v):
    v &= 0xffffffff
    return v - (1 << 32) if v >> 31 else v


def _codes(tr, net, i, what):
    """op i's word with the chain bits 24..27 set to 0 and then to every other code, one call each (a code that has no form for that
    chain is refused: the snapshot then shows that nothing moved), and back to the word it had"""
    w = net.choices()[i]
    for code in range(16):
        rc = _set(net, i, _signed((w & ~(15 << 24)) | (code << 24)))
        tr.rec("%s: op %d code %d" % (what, i, code), net, rc)
    tr.rec("%s: op %d restored" % (what, i), net, _set(net, i, w))


def _only_res4(net, i0):
    ch = net.choices()
    for i, _, _ in net.stages():
        ch[i] = _signed(ch[i] | (1 << 30)) if i == i0 else _signed(ch[i] & ~(1 << 30) & 0x7fffffff)
    net.set_choices(ch)


# ------------------------------------------------------------------------------------------------------------------------------ the walks
def walk_resnet50_stage():
    """ResNet50 INT8, batch 3, 96x96, stage=True (tests/test_gpu_stage_tail._resnet50)"""
    import numpy as np
    import torch
    from anakin_amd import lib as L
    from anakin_amd import workloads as W
    from tests import test_gpu_stage_tail as TT
    batch, hw = 3, 96
    model, scales, x, ref = TT._resnet50(batch, hw)
    tr = Trace()

    def build():
        return W.build_int8_net(model, dict(scales), batch, hw=hw, stage=True)

    def forward(n, what):
        n.tensor("data").copy_(torch.from_numpy(x).cuda())
        n.run()
        torch.cuda.synchronize()
        n.status()
        got = TT.host(n.tensor("fc1000"))
        assert np.array_equal(got, ref["fc1000"].reshape(got.shape)), what

    net = build()
    tr.rec("build", net)
    forward(net, "build")
    # the selectors
    net.select_stages(True)
    tr.rec("stages on", net)
    res4 = [s for s in net.stages() if net.op_name(s[0]).startswith("conv:stage_c256")]
    assert len(res4) == 1, net.stages()
    i0, nb = res4[0][0], res4[0][1]
    ip = int(L.load().saber_hip_net_stage_head(net.h, i0))
    it = i0 + 3 * nb
    assert ip == i0 - 1
    for on in (True, False, True):
        net.select_tails(on)
        tr.rec("tails %s" % on, net)
    forward(net, "stages + tails")
    for on in (True, False):
        net.select_heads(on)
        tr.rec("heads %s" % on, net)
        forward(net, "heads %s" % on)
    # heads on, then stages off, then stages on
    net.select_heads(True)
    tr.rec("heads on again", net)
    net.select_stages(False)
    tr.rec("stages off under the heads", net)
    forward(net, "stages off")
    net.select_stages(True)
    tr.rec("stages on after the heads", net)
    forward(net, "stages on again")
    # every chain decision, one op at a time: with every stage off, and with res4 selected
    for state in ("stages off", "res4 selected"):
        if state == "stages off":
            net.select_stages(False)
        else:
            _only_res4(net, i0)
        tr.rec(state, net)
        sites = [i for i, c in enumerate(net.choices()) if (c >> 28) & 3]
        assert len(sites) >= 20 and it in sites, sites
        for i in sites:
            _codes(tr, net, i, state)
        forward(net, state)
    # the strided head behind res4 while it runs as the tail (and the pair in front as the head)
    net.select_tails(True)
    assert net.tails() == [(i0, nb)], net.tails()
    tr.rec("res4 with its tail", net)
    _codes(tr, net, it, "tail on")
    net.select_heads(True)
    tr.rec("res4 with tail and head", net)
    for i in (it, it + 1, ip, i0):
        _codes(tr, net, i, "tail and head on")
    forward(net, "tail and head on")
    # the pair's word asks for the head while the stage is off; the stage's own word comes next
    net.select_stages(True)
    net.select_tails(True)
    net.select_heads(True)
    tr.rec("every stage, tail and head on", net)
    ch_all_on = net.choices()
    net.select_stages(False)
    ch_all_off = net.choices()
    tr.rec("stages off before the pair's word", net)
    tr.rec("pair word, bit 29", net, _set(net, ip, ch_all_off[ip] | (1 << 29)))
    tr.rec("stage word", net, _set(net, i0, ch_all_off[i0] | (1 << 30)))
    forward(net, "pair word, then stage word")
    tr.rec("stage word with the tail bit", net, _set(net, i0, _signed(ch_all_off[i0] | (3 << 30))))
    tr.rec("stage word off", net, _set(net, i0, ch_all_off[i0]))
    tr.rec("stage word alone", net, _set(net, i0, ch_all_off[i0] | (1 << 30)))
    forward(net, "stage word alone")
    # the whole list of the everything-on state to a fresh net and back
    fresh = build()
    tr.rec("fresh", fresh)
    fresh.set_choices(ch_all_on)
    tr.rec("fresh: everything on", fresh)
    forward(fresh, "fresh: everything on")
    fresh.set_choices(ch_all_off)
    tr.rec("fresh: everything off", fresh)
    fresh.set_choices(ch_all_on)
    tr.rec("fresh: everything on again", fresh)
    forward(fresh, "fresh: everything on again")
    # a stage launch that did not complete, with stage, tail and head on
    net.set_choices(ch_all_on)
    tr.rec("everything on", net)
    assert net.heads() and net.tails()
    L.check(L.load().saber_hip_net_inject_coop_error(net.h))
    try:
        net.status()
    except L.SaberHipError:
        pass
    else:
        raise AssertionError("status() did not report the injected error")
    tr.rec("after the failed stage launch", net)
    forward(net, "after the failed stage launch")
    return tr.steps


def walk_resnet50_head_pair():
    """the same model through the Python builder with the strided head + pair launch (flag 1024) and the stem pair (flag 512)"""
    from tests import py_fuser as PF
    from tests import test_gpu_stage_tail as TT
    model, scales, _, _ = TT._resnet50(3, 96)
    tr = Trace()
    net = PF.build_int8_net(model, dict(scales), 2, head_pair=True)
    tr.rec("build", net)
    names = [net.op_name(i) for i in range(net.num_ops())]
    assert sum("+pair1x1_c" in n for n in names) == 1 and sum(n == "conv:(in the stem launch)" for n in names) == 1, names
    for i, c in enumerate(net.choices()):
        if (c >> 29) & 1:
            tr.rec("led chain %d off" % i, net, _set(net, i, c & ~(15 << 24)))
            tr.rec("led chain %d on" % i, net, _set(net, i, c))
    sp = names.index("conv:(in the stem launch)")
    w = net.choices()[sp]
    tr.rec("the stem pair op's word", net, _set(net, sp, (w or 1) | (1 << 29)))
    tr.rec("the stem op's word", net, _set(net, sp - 1, net.choices()[sp - 1] or 1))
    return tr.steps


def walk_mobilenet_sep():
    """MobileNet-v1 INT8, batch 3, 96x96, separable=True (tests/test_gpu_sep.test_choice_round_trip's net)"""
    from anakin_amd import workloads as W
    model = W.build_model("mobilenet_v1")
    fw = W.framework_model(model, "int8")
    scales = W.calibrate(model, W.make_input(3, hw=96))
    tr = Trace()

    def build():
        return W.build_int8_net(fw, dict(scales), 3, hw=96, separable=True)

    net = build()
    tr.rec("build", net)
    sites = [i for i, c in enumerate(net.choices()) if (c >> 28) & 3 == 3]
    assert len(sites) == 13, sites
    for i in sites:
        tr.rec("site %d off" % i, net, _set(net, i, net.choices()[i] & ~(15 << 24)))
    for i in sites:
        _codes(tr, net, i, "separable")
    for k, i in enumerate(sites):      # every other site on, with its first form
        if k % 2 == 0:
            w = net.choices()[i] & ~(15 << 24)
            assert any(_set(net, i, w | (code << 24)) == 0 for code in range(1, 16)), i
    tr.rec("every other site on", net)
    for i in sites:
        tr.rec("site %d: a word without the separable bits" % i, net, _set(net, i, net.choices()[i] & 0xffffff))
    ch = net.choices()
    fresh = build()
    tr.rec("fresh", fresh)
    fresh.set_choices(ch)
    tr.rec("fresh: the walked net's choices", fresh)
    return tr.steps


WALKS = {"resnet50_stage": walk_resnet50_stage, "resnet50_head_pair": walk_resnet50_head_pair, "mobilenet_sep": walk_mobilenet_sep}
