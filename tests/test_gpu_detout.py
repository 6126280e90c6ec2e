"""The DetectionOutput op on the GPU (anakin_amd/csrc/detout.hip): both forms on every case of tests/detout_util.py against the float32
restatement (which tests/test_detout_cpu.py ties to the reference's own recorded outputs): columns 0 - 2, the row order, the padding rows
and `count` with `==` everywhere, the box columns too - CENTER_SIZE's, behind the one transcendental, included: the device's largest
difference from the recorded reference was measured as 0 (test_center_size_boxes_against_the_recording prints it;
profiles/detout/README.md), so equality is asserted in place of the FP32 bound; the two forms `==` each other; chunked selection one above the sorting capacity; guard bands; dirty buffers; an SSD head through the executor
eagerly, replayed, autotuned and replayed with fresh inputs; the op-list capture."""
import os
import subprocess

import numpy as np
import pytest
import torch

from anakin_amd import lib as L
from anakin_amd import saber as S
from oracle import oracle as O
from tests import detout_util as DU
from tests import guard_util as GU

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "detout_ref.npz"))
NAMES = ["detout_direct_f32", "detout_mask_f32"]
CASES = sorted(DU.GOLDEN_CASES)
_REF = {}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


inputs = DU.inputs


def ref(name):
    """the restatement's (y, count) of a recorded case, computed once"""
    if name not in _REF:
        y, c = DU.detout_ref(DU.GOLDEN_CASES[name], *inputs(name))
        y.setflags(write=False)
        c.setflags(write=False)
        _REF[name] = (y, c)
    return _REF[name]


def make_op(cs):
    return S.SaberDetectionOutput(cs["n"], cs["c"], cs["p"], cs["keep"], cs["nms_k"], cs["conf_t"], cs["nms_t"], cs["bg"], cs["code"], cs["vit"],
                                  cs["prior"], cs["eta"])


def run(op, loc, conf, prior, form, y=None, count=None):
    op.set_tile(form)
    assert op.algo() == NAMES[form] and op.tile() == form
    if y is None:
        y, count = op.new_outputs()
        y.fill_(float("nan"))
        count.fill_(77)
    op.run(dev(loc), dev(conf), None if prior is None else dev(prior), y, count)
    return host(y), host(count)


def check(got, want, what, code=DU.CORNER):
    """every column, the row order, the padding rows and count `==`. CENTER_SIZE too: the device's largest difference from the recorded
    reference was measured as 0 (profiles/detout/README.md), so equality is asserted in place of the FP32 bound"""
    (y, c), (wy, wc) = got, want
    assert c.tolist() == wc.tolist(), (what, c.tolist(), wc.tolist())
    assert DU.same_bits(y[:, :3], wy[:, :3]), (what, "image / label / score columns or the row order")
    d = np.abs(y[:, 3:].astype(np.float64) - wy[:, 3:].astype(np.float64))
    assert DU.same_bits(y[:, 3:], wy[:, 3:]), (what, "box columns, code type %d, largest difference %g" % (code, float(np.nanmax(d))))


@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("name", CASES)
def test_case_against_the_restatement(name, form):
    cs = DU.GOLDEN_CASES[name]
    op = make_op(cs)
    if form == 1 and cs["eta"] < 1:
        with pytest.raises(L.SaberHipError):
            op.set_tile(1)
        assert op.tile() == 0 and op.forms() == [0]
        return
    assert op.forms() == ([0] if cs["eta"] < 1 else [0, 1]) and op.out_rows() == cs["n"] * cs["keep"]
    got = run(op, *inputs(name), form)
    check(got, ref(name), name, cs["code"])
    if form == 1:      # the forms are bit-identical to each other
        other = run(op, *inputs(name), 0)
        assert DU.same_bits(got[0], other[0]) and DU.same_bits(got[1], other[1])


def test_center_size_boxes_against_the_recording():
    """the device's CENTER_SIZE boxes against the boxes the reference itself decoded: every decoded box that reaches an output row"""
    worst = 0.0
    for name in CASES:
        cs = DU.GOLDEN_CASES[name]
        if cs["code"] != DU.CENTER_SIZE:
            continue
        y, c = run(make_op(cs), *inputs(name), 0)
        rows = GOLDEN[name + "/rows"]
        assert c[0] == len(rows)
        assert DU.same_bits(y[:len(rows), :3], rows[:, :3])
        d = np.abs(y[:len(rows), 3:].astype(np.float64) - rows[:, 3:].astype(np.float64)).max() / np.abs(rows[:, 3:]).max()
        worst = max(worst, float(d))
    print("largest relative difference of a CENTER_SIZE box from the recorded reference:", worst)
    assert worst == 0.0


def _big(n, c, p, keep, nms_k, seed, disjoint):
    cs = DU.case(n, c, p, prior=False, bg=-1, keep=keep, nms_k=nms_k, conf_t=0.0, special="disjoint" if disjoint else None)
    rng = np.random.default_rng(seed)
    loc, conf, _ = DU.make(cs, rng)
    conf = (conf * np.float32(0.5) + np.float32(0.25)).astype(np.float32)      # every score above the threshold
    return cs, loc, conf


@pytest.mark.parametrize("form", [0, 1])
def test_one_prior_above_the_sorting_capacity(form):
    """P = DETOUT_SORT_CAP + 1, two classes, every score a candidate: the running top-K is carried into a second sort"""
    key = "cap"
    if key not in _REF:
        cs, loc, conf = _big(1, 2, DU.SORT_CAP + 1, 12, 24, 5, False)
        conf[0, :, -1] = np.float32(0.99)      # the last prior, alone in its chunk, leads both classes
        _REF[key] = (cs, loc, conf, DU.detout_ref(cs, loc, conf, None))
    cs, loc, conf, want = _REF[key]
    assert want[0][0, 2] == np.float32(0.99)
    check(run(make_op(cs), loc, conf, None, form), want, "P = %d" % cs["p"])


def test_keep_top_k_cut_over_more_kept_boxes_than_one_sort_holds():
    """five classes keep 1024 disjoint boxes each: the per-image selection sorts twice"""
    cs, loc, conf = _big(1, 5, 1030, 3000, 1024, 6, True)
    want = DU.detout_ref(cs, loc, conf, None)
    assert want[1].tolist() == [3000, 3000]
    op = make_op(cs)
    got = run(op, loc, conf, None, 1)
    check(got, want, "5 x 1024 kept, keep_top_k 3000")
    assert DU.same_bits(run(op, loc, conf, None, 0)[0], got[0])


@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("name", ["corner", "noprior", "keeps_nothing", "all_rows_filled", "center_300"])
def test_between_guard_bands(name, form):
    cs = DU.GOLDEN_CASES[name]
    op = make_op(cs)
    op.set_tile(form)
    loc, conf, prior = inputs(name)

    def launch(T, ws):
        op.run(T["loc"], T["conf"], T["prior"], T["y"], T["count"])

    def plain(ins, outs, ws_bytes):
        T = {k: (None if v is None else dev(v)) for k, v in ins.items()}
        T["y"], T["count"] = op.new_outputs()
        return T, None
    got = GU.run_guarded({"loc": loc, "conf": conf, "prior": prior},
                         {"y": ((op.out_rows(), 7), np.float32, None), "count": ((1 + cs["n"],), np.int32, None)}, launch, plain=plain,
                         what="%s form %d" % (name, form))
    check((got["y"], got["count"]), ref(name), name, cs["code"])


@pytest.mark.parametrize("form", [0, 1])
def test_second_run_into_dirty_buffers(form):
    """the outputs (and the op's scratch) hold another case's result: the run rewrites every byte it owns"""
    big = "all_rows_filled"
    a = DU.GOLDEN_CASES[big]
    op = make_op(a)
    y, count = op.new_outputs()
    y.fill_(float("nan"))
    first = run(op, *inputs(big), form, y, count)
    check(first, ref(big), big)
    again = run(op, *inputs(big), form, y, count)
    assert DU.same_bits(first[0], again[0]) and DU.same_bits(first[1], again[1])
    # the same op and buffers, inputs that keep far fewer rows (every score of image 1 below the threshold): no stale row survives
    loc, conf, prior = inputs(big)
    conf2 = conf.copy()
    conf2[1] = np.float32(-1.0)
    want = DU.detout_ref(a, loc, conf2, prior)
    assert want[1][2] == 0 and want[1][0] < first[1][0]
    check(run(op, loc, conf2, prior, form, y, count), want, "fewer rows into the same buffers")


def test_set_tile_round_trip():
    op = make_op(DU.GOLDEN_CASES["corner"])
    start = op.tile()
    assert op.algo() == NAMES[start]
    for f in (1, 0, 1):
        op.set_tile(f)
        assert op.tile() == f and op.algo() == NAMES[f]
    with pytest.raises(L.SaberHipError):
        op.set_tile(2)
    assert op.tile() == 1


# ---- an SSD head through the executor ---------------------------------------------------------------------------------------------------
A, CLS, CIN = 2, 4, 8      # anchors per position, classes, feature channels
MAPS = ((6, 6), (3, 3))
PRI = sum(h * w for h, w in MAPS) * A


def ssd_params():
    rng = np.random.default_rng(20)

    def wb(k, scale):
        return (rng.standard_normal((k, CIN, 3, 3)) * scale).astype(np.float32), (rng.standard_normal(k) * 0.1).astype(np.float32)
    convs = {"loc0": wb(A * 4, 0.05), "conf0": wb(A * CLS, 0.2), "loc1": wb(A * 4, 0.05), "conf1": wb(A * CLS, 0.2)}
    boxes = []
    for h, w in MAPS:
        for i in range(h):
            for j in range(w):
                for a in range(A):
                    cx, cy, s = (j + 0.5) / w, (i + 0.5) / h, (0.9 + 0.5 * a) / w
                    boxes.append([cx - s / 2, cy - s / 2, cx + s / 2, cy + s / 2])
    prior = np.stack([np.array(boxes, np.float32).reshape(-1), np.tile(np.array([0.1, 0.1, 0.2, 0.2], np.float32), PRI)])
    return convs, prior


def ssd_inputs(n, seed):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal((n, CIN, h, w)).astype(np.float32) for h, w in MAPS]


def ssd_case(n):
    return DU.case(n, CLS, PRI, code=DU.CENTER_SIZE, bg=0, keep=10, nms_k=40, conf_t=0.3, nms_t=0.45)


def ssd_net(n):
    convs, prior = ssd_params()
    cs = ssd_case(n)
    net = S.Net()
    for m, (h, w) in enumerate(MAPS):
        net.add_tensor("x%d" % m, (n, h, w, CIN), L.F32)
        net.add_tensor("loc%d" % m, (n, h * w * A * 4), L.F32)      # the NHWC conv output IS the permuted, flattened head
        net.add_tensor("conf%d" % m, (n, h * w * A * CLS), L.F32)
    for nm, shape in (("loc", (n, PRI * 4)), ("logit", (n, PRI * CLS)), ("conf", (n, PRI * CLS)), ("prior", (2, PRI * 4)),
                      ("y", (n * cs["keep"], 7)), ("count", (1 + n,))):
        net.add_tensor(nm, shape, L.F32)
    idx = {}
    for m, (h, w) in enumerate(MAPS):
        for head in ("loc", "conf"):
            wt, b = convs["%s%d" % (head, m)]
            conv = S.SaberConv2D(False).init((n, CIN, h, w), S.ConvParam(wt, b, 1, (1, 1), (1, 1), (1, 1), False), L.F32, L.F32, in_layout=L.NHWC,
                                             out_layout=L.NHWC)
            idx["%s%d" % (head, m)] = net.add_conv(conv, "x%d" % m, "%s%d" % (head, m))
    idx["loc"] = net.add_concat(["loc0", "loc1"], "loc")
    idx["logit"] = net.add_concat(["conf0", "conf1"], "logit")
    idx["conf"] = net.add_softmax(n * PRI, CLS, "logit", "conf")
    op = make_op(cs)
    idx["y"] = net.add_detout(op, "loc", "conf", "prior", "y", "count")
    net.finalize()
    return net, cs, idx, op, convs, prior


def ssd_fill(net, xs, prior):
    for nm in net.tensors:
        net.tensor(nm).fill_(float("nan"))
    for m, x in enumerate(xs):
        net.tensor("x%d" % m).copy_(dev(np.ascontiguousarray(x.transpose(0, 2, 3, 1))))
    net.tensor("prior").copy_(dev(prior))


def ssd_check(net, cs, xs, convs, prior, what):
    """every edge: the convs against the oracle's FP32 conv (the project's FP32 bound), the concats and the softmax against the edges they
    read, the detout `==` the restatement of the loc / conf edges the device itself produced"""
    n = cs["n"]
    e = {nm: host(net.tensor(nm)).copy() for nm in net.tensors}
    for m, (h, w) in enumerate(MAPS):
        for head in ("loc", "conf"):
            wt, b = convs["%s%d" % (head, m)]
            want = O.conv_f32_nchw(xs[m], wt, b, False, (1, 1), (1, 1)).transpose(0, 2, 3, 1).reshape(n, -1)
            got = e["%s%d" % (head, m)]
            assert float(np.abs(got - want).max() / np.abs(want).max()) <= 1e-4, (what, head, m)
    assert DU.same_bits(e["loc"], np.concatenate([e["loc0"], e["loc1"]], 1)), what
    assert DU.same_bits(e["logit"], np.concatenate([e["conf0"], e["conf1"]], 1)), what
    lg = e["logit"].reshape(n * PRI, CLS).astype(np.float64)
    sm = np.exp(lg - lg.max(1, keepdims=True))
    sm /= sm.sum(1, keepdims=True)
    assert float(np.abs(e["conf"].reshape(n * PRI, CLS) - sm).max()) <= 1e-5, what
    want = DU.detout_ref(cs, e["loc"], e["conf"].reshape(n, PRI, CLS), prior)
    check((e["y"], e["count"].view(np.int32)), want, what, cs["code"])
    return want


@pytest.mark.parametrize("n", [1, 3])
def test_ssd_head_eager_replayed_and_autotuned(n):
    net, cs, idx, op, convs, prior = ssd_net(n)
    i = idx["y"]
    assert net.num_ops() == net.num_launches() == 8
    assert net.op_name(i) == "detout:" + op.algo() and net.choices()[i] == (20 << 16) | op.tile()
    nbytes, flops = net.op_work(i)
    assert nbytes > 4.0 * n * PRI * CLS and flops > 0
    xs = ssd_inputs(n, 1)
    ssd_fill(net, xs, prior)
    net.run()
    want = ssd_check(net, cs, xs, convs, prior, "eager")
    assert 0 < want[1][0]
    ssd_fill(net, xs, prior)
    net.capture()
    net.replay()
    ssd_check(net, cs, xs, convs, prior, "replayed")
    # the op on its own, each form through the choice word: the same bytes
    first = None
    for form in (1, 0):
        ch = net.choices()
        ch[i] = (20 << 16) | form
        net.set_choices(ch)
        assert net.choices()[i] == (20 << 16) | form and net.op_name(i) == "detout:" + NAMES[form]
        net.tensor("y").fill_(float("nan"))
        net.tensor("count").fill_(float("nan"))
        net.run_op(i)
        got = (host(net.tensor("y")).copy(), host(net.tensor("count")).view(np.int32).copy())
        check(got, want, "run_op, form %d" % form, cs["code"])
        first = got if first is None else first
        assert DU.same_bits(got[0], first[0])
    ch = net.choices()
    ch[i] = (20 << 16) | 5
    with pytest.raises(L.SaberHipError):
        net.set_choices(ch)
    assert net.op_name(i) == "detout:" + NAMES[0]
    ssd_fill(net, xs, prior)
    net.run()
    net.autotune(3)
    tuned = net.choices()[i]
    assert tuned >> 16 == 20 and (tuned & 0xff) in (0, 1) and net.op_name(i) == "detout:" + NAMES[tuned & 0xff]
    ssd_fill(net, xs, prior)
    net.capture()
    net.replay()
    ssd_check(net, cs, xs, convs, prior, "autotuned, replayed")


def test_ssd_head_ten_replays_with_fresh_inputs():
    n = 2
    net, cs, idx, op, convs, prior = ssd_net(n)
    xs = ssd_inputs(n, 100)
    ssd_fill(net, xs, prior)
    net.capture()
    seen = set()
    for k in range(10):
        xs = ssd_inputs(n, 100 + k)
        for m, x in enumerate(xs):
            net.tensor("x%d" % m).copy_(dev(np.ascontiguousarray(x.transpose(0, 2, 3, 1))))
        net.replay()      # no recapture
        seen.add(ssd_check(net, cs, xs, convs, prior, "replay %d" % k)[0].tobytes())
    assert len(seen) == 10      # every replay detected something else: the graph read the fresh inputs


def test_detout_is_recorded_by_the_op_list_capture():
    name = "corner"
    cs = DU.GOLDEN_CASES[name]
    op = make_op(cs)
    loc, conf, prior = (dev(a) for a in inputs(name))
    y, count = op.new_outputs()
    y.fill_(123.0)
    with S.Capture() as cap:
        op.run(loc, conf, prior, y, count)
    assert float(host(y).min()) == 123.0 == float(host(y).max())      # recorded, not launched
    net = cap.net
    assert net.num_ops() == 1 and net.op_name(0) == "detout:" + op.algo()
    net.bind(net.tensor_of_ptr(y), y)
    net.bind(net.tensor_of_ptr(count), count)
    net.finalize()
    net.run()
    check((host(y), host(count)), ref(name), "op-list capture")


def test_saber_detection_output_through_the_stand_in_cpp_driver():
    """tests/cpp/test_saber_detout.cpp: SaberDetectionOutput<MI355X, AK_FLOAT> init -> dispatch under the stand-in Saber headers, the
    reshaped output outside an op-list capture and the capacity shape inside one"""
    exe = os.path.join(ROOT, "tests", "cpp", "test_saber_detout.bin")
    assert os.path.exists(exe), "tests/cpp/test_saber_detout.bin is missing: run __graft_entry__.build()"
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = os.pathsep.join([os.path.join(ROOT, "anakin_amd"), os.path.join(ROOT, "oracle"), env.get("LD_LIBRARY_PATH", "")])
    p = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0 and "detout cases ok" in p.stdout, p.stdout[-3000:] + p.stderr[-2000:]
