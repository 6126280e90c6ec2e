"""saber_hip_net_optimize on op lists where its rewrites must NOT apply (tests/oplist_util.py: the patterns, the perturbations, the oracle walk
in list order). The model builders only make lists in which every intermediate tensor has exactly the readers its pattern expects, is written
once and is never written in place; the C ABI accepts more, and the rewrites' side conditions ("the only reader", "nothing between the two
positions touches the tensor", "the residual exists before the conv runs", "lane 0", "no op belongs to two sites") decide about those.

Per pattern: the CONTROL (unperturbed: rewritten as today - return values, op count, launch count, unwritten set) and every perturbed case:
  (a) structure, before anything is launched: every tensor somebody outside the pattern sees (oplist_util.required) has storage and is
      reported written in every selectable form of the sites present. A list that fails (a) is never run.
  (b) values: eager, after autotune(iters = 2), replayed as a hipGraph, after compact() - every non-input poisoned before each run, every
      tensor of (a) plus every tensor the net reports written compared with the oracle walk byte for byte (1e-4 of the row maximum for a
      softmax output, 1e-4 of the largest magnitude for the f32 average pooling, as elsewhere in the suite); after compact() the outputs only.
  (c) each site's choice set to each of its forms, (b)'s eager and replayed runs repeated.
How a list declined is not asserted: a rewrite that stays legal under a perturbation may still apply. tests/test_oplist_cpu.py shows from
the oracle alone that each perturbed case would give other bytes (>= a quarter of a compared tensor) had the rewrite been applied anyway."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from anakin_amd import lib as L  # noqa: E402
from tests import oplist_util as U  # noqa: E402

POISON = U.POISON


@pytest.fixture(scope="module", autouse=True)
def _device():
    L.require_device()  # fail loudly: no fallback path exists


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


_want = {}


def oracle_of(key, desc, inputs):
    """the oracle walk of a case, computed once per module"""
    if key not in _want:
        _want[key] = U.run_oracle(desc, inputs)[0]
    return _want[key]


# ---- selections ----------------------------------------------------------------------------------------------------------------------------
def absorbed(net):
    return sum(1 for i in range(net.num_ops()) if "(in the " in net.op_name(i))


def site_ops(net):
    """[(op index, kind)] of the ops whose choice word records a site decision (saber_hip_net_get_choice)"""
    out = []
    for i, c in enumerate(net.choices()):
        c &= 0xffffffff
        if (c >> 30) == 2:
            out.append((i, "block"))          # an inverted-residual or a Fire site (bit 31 without bit 30)
        elif (c >> 28) & 3 == 3 and not (c >> 30):
            out.append((i, "sep"))
        elif (c >> 28) & 3 and not (c >> 31):
            out.append((i, "chain"))          # bit 28: a 1x1 chain, bit 29: a 3x3-led chain
    return out


def selections(net):
    """every selectable form of the sites present, one site changed at a time from the static selection (the _all_modes idea of
    test_gpu_resnet.py): [(label, choices)]; form codes the site does not have are refused by set_choice and passed by"""
    lib, base = L.load(), net.choices()
    out = [("static", base)]
    for i, kind in site_ops(net):
        for code in range(16):
            word = (base[i] & ~(15 << 24)) | (code << 24)
            if word == base[i]:
                continue
            if lib.saber_hip_net_set_choice(net.h, i, word) == 0:
                ch = net.choices()
                if all(ch != c for _, c in out):
                    out.append(("op %d %s form %d" % (i, kind, code), ch))
            net.set_choices(base)
    for stages in (net.stages(), net.stages_c64()):
        for i, _, on in stages:
            ch = list(base)
            ch[i] = (ch[i] & ~(1 << 30)) if on else (ch[i] | (1 << 30))
            net.set_choices(ch)
            out.append(("op %d stage %s" % (i, "off" if on else "on"), net.choices()))
            net.set_choices(base)
    assert net.choices() == base
    return out


# ---- (a) structure ---------------------------------------------------------------------------------------------------------------------------
def storage_problems(net, desc):
    lib = L.load()
    return ["%s has no storage" % nm for nm in U.required(desc) if lib.saber_hip_net_tensor_bytes(net.h, net.tid(nm)) == 0]


def unwritten_problems(net, desc, forms):
    bad, base = [], net.choices()
    for label, ch in forms:
        net.set_choices(ch)
        bad += ["%s is not written (%s)" % (nm, label) for nm in U.required(desc) if net.unwritten(nm)]
    net.set_choices(base)
    return bad


def build(desc, flags):
    """the net of a description, optimised and - only when (a) holds - finalized: (net, return values, selectable forms)"""
    net, rets = U.build_net(desc, flags)
    bad = storage_problems(net, desc)
    assert not bad, bad      # (a): a list with a zero-byte output is never launched
    net.finalize()
    forms = selections(net)
    bad = unwritten_problems(net, desc, forms)
    assert not bad, bad
    return net, rets, forms


# ---- (b) values ------------------------------------------------------------------------------------------------------------------------------
def _tolerances(desc):
    """{name: None (byte for byte) | "row" (softmax) | "max" (the f32 average pooling and copies of it)}"""
    tol = {}
    for o in desc.ops:
        if o["kind"] == "softmax":
            tol[o["out"]] = "row"
        elif o["kind"] == "gpool_f32":
            tol[o["out"]] = "max"
        elif o["kind"] == "concat" and any(tol.get(t) for t in o["ins"]):
            tol[o["out"]] = "max"
    return tol


def fill(net, desc, inputs):
    lib = L.load()
    for nm, (shape, dt) in desc.tensors.items():
        if nm in desc.inputs:
            net.tensor(nm).copy_(dev(inputs[nm]))
        elif lib.saber_hip_net_tensor_bytes(net.h, net.tid(nm)):      # (a removed edge has no bytes of its own to poison)
            net.tensor(nm).fill_(float("nan") if dt == U.F32 else POISON)


def check(net, desc, want, names, what):
    tol = _tolerances(desc)
    for nm in names:
        got, w = host(net.tensor(nm)), want[nm]
        if tol.get(nm) == "row":
            assert np.all(np.abs(got - w).max(axis=-1) <= 1e-4 * w.max(axis=-1)), (what, nm)
        elif tol.get(nm) == "max":
            assert np.abs(got - w).max() <= 1e-4 * np.abs(w).max(), (what, nm)
        else:
            assert got.dtype == w.dtype and np.array_equal(got, w), (what, nm, int(np.count_nonzero(got != w)), w.size)


def live_names(net, desc):
    lib = L.load()
    need = U.required(desc)
    return need + [nm for nm in U.written(desc) if nm not in need and lib.saber_hip_net_tensor_bytes(net.h, net.tid(nm)) and not net.unwritten(nm)]


def passes(net, desc, inputs, want, what, modes=("eager", "replayed")):
    for mode in modes:
        fill(net, desc, inputs)
        if mode == "eager":
            net.run()
        else:
            net.capture()
            net.replay()
        torch.cuda.synchronize()
        net.status()
        check(net, desc, want, live_names(net, desc), (what, mode))


def values(net, desc, inputs, want, forms, what, tune=True, compact=True):
    passes(net, desc, inputs, want, (what, "static"))
    if tune:
        fill(net, desc, inputs)
        net.run()
        net.autotune(iters=2)
        passes(net, desc, inputs, want, (what, "autotuned"))
        net.set_choices(forms[0][1])
    for label, ch in forms[1:]:      # (c)
        net.set_choices(ch)
        passes(net, desc, inputs, want, (what, label))
    net.set_choices(forms[0][1])
    if compact:
        net.compact()      # (no keep list: inner edges hold garbage from here on; a fresh run from the inputs)
        for nm in desc.inputs:
            net.tensor(nm).copy_(dev(inputs[nm]))
        for nm in U.unread(desc):
            net.tensor(nm).fill_(float("nan") if desc.tensors[nm][1] == U.F32 else POISON)
        net.run()
        torch.cuda.synchronize()
        net.status()
        check(net, desc, want, U.unread(desc), (what, "compacted"))


# ---- the control ---------------------------------------------------------------------------------------------------------------------------
# pattern -> (optimize return values in oplist_util.flags_for's order, ops, launches and unwritten edges with every site's one launch selected)
CONTROL = {
    "f1": ([1], 1, 1, {"t"}),                       # conv + eltwise: one op, its own edge gone
    "f4": ([1], 1, 1, {"t"}),                       # stem conv + pooling
    "f128": ([1], 1, 1, set()),                     # conv + global pooling: one launch, both tensors written
    "f2": ([1], 1, 1, set()),                       # the sibling pair
    "f64": ([1, 1], 1, 1, {"t", "q"}),              # conv + eltwise, the shortcut pooling folded into its residual read
    "tail": ([1, 1], 3, 2, set()),                  # pooling writes the fc's operand; fc + softmax in one launch
    "sep": ([1], 2, 1, {"m"}),
    "ir": ([1, 1], 3, 1, {"p", "e", "d"}),
    "fire": ([1], 4, 1, {"s", "a", "b"}),
    "chain": ([2, 4], 6, 2, {"t1_0", "t1_1", "t0_0", "t0_1"}),      # two eltwise sums fused; two 3x3-led chains
    "f512": ([2, 1], 2, 1, {"t", "u"}),             # conv + pooling and the pair; then the stem launch runs the pair
    "head": ([2, 1, 2], 3, 1, {"q", "t1", "t0"}),      # eltwise + pair; the shortcut pooling folded; conv3x3 + conv1x1 + the pair in one launch
    "stage": ([2, 4], 6, 1, {"t1_0", "t1_1", "t0_0", "t0_1", "y1_0"}),      # ... and the C = 64 stage: the inner block output stays in LDS
}


def all_sites_on(net, forms):
    """the selection with the most ops absorbed among the selectable forms (each site's one launch on)"""
    best = None
    for label, ch in forms:
        net.set_choices(ch)
        n = net.num_launches()
        if best is None or n < best[0]:
            best = (n, ch)
    net.set_choices(forms[0][1])
    return best[1]


@pytest.mark.parametrize("name", sorted(U.PATTERNS))
def test_control_pattern_is_rewritten_as_today(name):
    desc, inputs, pat = U.pattern(name)
    want = oracle_of((name, "control"), desc, inputs)
    net, rets, forms = build(desc, U.flags_for([pat]))
    exp_rets, exp_ops, exp_launches, exp_unwritten = CONTROL[name]
    print(name, "optimize ->", rets, [net.op_name(i) for i in range(net.num_ops())], [f[0] for f in forms])
    assert rets == exp_rets and net.num_ops() == exp_ops, (name, rets, net.num_ops())
    if site_ops(net) or name == "f512":
        with pytest.raises(L.SaberHipError):      # launches that span several ops' tensors exist: no lane change any more
            net.set_lane(0, 1)
    net.set_choices(all_sites_on(net, forms))
    assert net.num_launches() == exp_launches and net.num_launches() + absorbed(net) == net.num_ops(), (name, net.num_launches(), absorbed(net))
    assert {nm for nm in desc.tensors if net.unwritten(nm)} == exp_unwritten, (name, [nm for nm in desc.tensors if net.unwritten(nm)])
    net.set_choices(forms[0][1])
    values(net, desc, inputs, want, forms, name)


# ---- the perturbed cases -------------------------------------------------------------------------------------------------------------------
def _cases(names):
    return [(name, case) for name in names for case in U.perturbations(name)]


@pytest.mark.parametrize("name,case", _cases(sorted(U.PATTERNS)), ids=["%s-%s" % nc for nc in _cases(sorted(U.PATTERNS))])
def test_perturbed_list_keeps_its_bytes(name, case):
    _, _, pat = U.pattern(name)
    desc, inputs = U.perturbations(name)[case]
    want = oracle_of((name, case), desc, inputs)
    net, rets, forms = build(desc, U.flags_for([pat]))
    print(name, case, "optimize ->", rets, [net.op_name(i) for i in range(net.num_ops())], [f[0] for f in forms])
    if case.startswith("lane:"):
        # an op of the pattern on the side lane: no launch that spans several ops' tensors forms at all
        assert not site_ops(net) and not net.stages() and not net.stages_c64() and absorbed(net) == 0, (name, case, net.choices())
        if (case == "lane:" + pat.ops[0] and name in ("f1", "f128")) or name == "f2":      # flags 1, 2 and 128 want their convs on lane 0
            assert rets[0] == 0 and net.num_ops() == len(desc.ops), (name, case, rets)
    assert net.num_launches() + absorbed(net) == net.num_ops()
    values(net, desc, inputs, want, forms, (name, case), tune=not case.startswith("lane:"))


def test_the_stem_conv_cannot_leave_lane_0():
    """flag 4's conv pattern is the stem conv, which pads its three channels in the shared workspace: set_lane refuses it"""
    desc, inputs, pat = U.pattern("f4")
    d, _ = U.on_lane(desc, inputs, pat.ops[0])
    with pytest.raises(L.SaberHipError):
        U.build_net(d, [15])


# ---- ordering ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,first,second", [("irchain", U.IR, 16 | 32), ("irsep", U.IR, U.SEP)])
def test_site_flags_in_both_orders(name, first, second):
    """a list two site flags are offered at once: whichever comes first takes the ops, no op's launch is covered twice, the bytes are the
    same. irsep: the block flag and the separable flag both take the depthwise and the project conv. irchain: the ops the chain flag looks
    at (a fused-eltwise 1x1 conv and the 1x1 conv behind it) are a block's project conv and its follower; today's kernels never accept
    the same op twice there (a chain head is C -> 4C with its residual, a block's residual is its input with Cin <= 192), so what this
    order pins is that the chain flag, first or second, leaves the block's ops alone."""
    desc, inputs, pat = U.pattern(name)
    want = oracle_of((name, "control"), desc, inputs)
    formed = {}
    for order in ((first, second), (second, first)):
        net, rets, forms = build(desc, [15] + list(order))
        sites = site_ops(net)
        print(name, order, "optimize ->", rets, sites, [net.op_name(i) for i in range(net.num_ops())])
        formed[order] = sites
        if name == "irsep":      # exactly one site: the first flag's, and the second flag forms nothing over its ops
            assert rets[1:] == [1, 0] and sites == ([(0, "block")] if order[0] == U.IR else [(1, "sep")]), (order, rets, sites)
        for label, ch in forms:
            net.set_choices(ch)
            assert net.num_launches() + absorbed(net) == net.num_ops(), (name, order, label)
        net.set_choices(forms[0][1])
        values(net, desc, inputs, want, forms, (name, order), tune=False)
    assert all(formed.values()), (name, formed)      # (the list does match: each order forms a site)


# ---- random composition ----------------------------------------------------------------------------------------------------------------------
STARTERS = ["f1", "f4", "f64", "chain", "sep", "fire", "f2", "head"]
FOLLOWERS = ["f1", "f2", "sep", "fire", "ir", "tail", "irchain", "f128"]


def compose(seed):
    """3 to 5 patterns (the number drawn once) chained output to input - a pairing whose shapes do not fit is passed by and another drawn -
    and 0 to 3 (seed % 4) random perturbations of any kind"""
    rng = np.random.default_rng(5000 + seed)
    b = U.Builder(6000 + seed)
    fns = dict(U.PATTERNS, irchain=U.pat_irchain)
    want = int(rng.integers(3, 6))
    pats = [fns[STARTERS[rng.integers(len(STARTERS))]](b, "p0_")]
    for _ in range(200):
        if len(pats) >= want:
            break
        p = fns[FOLLOWERS[rng.integers(len(FOLLOWERS))]](b, "p%d_" % len(pats), pats[-1].out)
        if p is not None and (len(pats) + 1 >= want or b.d.tensors[p.out][1] != U.F32):      # (an f32 output ends the chain: last place only)
            pats.append(p)
    assert len(pats) == want >= 3, (seed, [p.name for p in pats])
    desc, inputs, done = b.d, {nm: b.val[nm] for nm in b.d.inputs}, []
    once = lambda kind: not any(d[1] == kind for d in done)      # (these perturbations name their new ops: one of a kind per list)
    for k in range(60):      # seed % 4 = 0 to 3 perturbations; a draw that does not apply to the pattern drawn is drawn again
        if len(done) >= seed % 4:
            break
        p = pats[rng.integers(len(pats))]
        what = ["reader", "in_place", "rewrite_before_use", "rewrite_source", "residual_late", "lane"][rng.integers(6)]
        r = None
        if what == "in_place" and p.elt and not any(d[0] == p.tag for d in done):
            side = int(rng.integers(2))
            r, label = U.in_place(desc, inputs, p, side), (p.tag, what, side)
        elif what == "rewrite_before_use" and p.moved and once(what) and not any(d[0] == p.tag for d in done):
            r, label = U.rewrite_before_use(desc, inputs, p), (p.tag, what)
        elif what == "rewrite_source" and p.source and once(what) and p.source[0] in desc.inputs:
            r, label = U.rewrite_source(desc, inputs, p), (p.tag, what)
        elif what == "residual_late" and p.late and once(what) and not any(d[0] == p.tag for d in done):
            r, label = U.residual_late(desc, inputs, p), (p.tag, what)
        elif what == "lane" and once(what):
            r, label = U.on_lane(desc, inputs, p.lane), (p.tag, what, p.lane)
        elif what == "reader" and p.inner:
            t = p.inner[rng.integers(len(p.inner))]
            pos = U.reader_positions(desc, p, t)
            where = sorted(pos)[rng.integers(len(pos))]
            kind = U.READER_KINDS[rng.integers(5)]
            r, label = U.extra_reader(desc, inputs, t, kind, pos[where], tag="xr%d" % k), (p.tag, "reader", t, kind, where)
        if r is not None:
            desc, inputs = r
            done.append(label)
    return desc, inputs, pats, done


@pytest.mark.parametrize("seed", range(8))
def test_random_composition(seed):
    desc, inputs, pats, done = compose(seed)
    want = oracle_of(("compose", seed), desc, inputs)
    flags = U.flags_for(pats)
    net, rets, forms = build(desc, flags)
    print("seed %d: %s; perturbed %s; optimize %s -> %s; sites %s; %d ops in %d launches: %s" %
          (seed, [p.name for p in pats], done, flags, rets, site_ops(net), net.num_ops(), net.num_launches(), [net.op_name(i) for i in range(net.num_ops())]))
    assert net.num_launches() + absorbed(net) == net.num_ops()
    passes(net, desc, inputs, want, ("compose", seed))


def test_interpreter_equals_the_branchy_net():
    """the interpreter's walk of test_gpu_fire._branchy_net's list equals that test's own reference, and the device's bytes"""
    from tests.test_gpu_fire import _branchy_net
    net, x, ref = _branchy_net(False)
    d, x2, _ = U.branchy_desc()
    assert np.array_equal(x, x2)
    got, _ = U.run_oracle(d, {"x": x})
    for nm in ref:
        assert np.array_equal(got[nm], ref[nm]), nm
    net.tensor("x").copy_(dev(x))
    net.run()
    for nm in ref:
        assert np.array_equal(host(net.tensor(nm)), ref[nm]), nm
