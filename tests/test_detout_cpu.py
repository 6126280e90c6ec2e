"""DetectionOutput without a GPU: the numpy restatement (tests/detout_util.py) against outputs recorded from the reference's own code
(tests/golden/detout_ref.npz, scripts/record_detout_golden.py), the closed-form keep_top_k order, the margin condition of the
CENTER_SIZE cases, descriptor validation, and proof that each injected defect is visible in some case. The second half: the cases of
DU.SCALE_CASES and the sweep (what tests/test_gpu_detout_scale.py runs on the device) each reach the boundary they are named for, and the
defects of DU.SCALE_DEFECTS change exactly the cases meant to show them."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import detout_util as DU

GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "detout_ref.npz"))
NAMES = sorted(DU.GOLDEN_CASES)
INVALID_VALUE = -2      # SABER_HIP_INVALID_VALUE


inputs = DU.inputs


def test_fixture_matches_the_case_table():
    """the fixture was recorded from the cases and the inputs this file's generator makes"""
    assert sorted({k.split("/")[0] for k in GOLDEN.files}) == NAMES
    for name in NAMES:
        cs = DU.GOLDEN_CASES[name]
        want = [float(cs[k]) for k in ("n", "c", "p", "code", "vit", "prior", "bg", "keep", "nms_k", "conf_t", "nms_t", "eta")]
        assert GOLDEN[name + "/param"].tolist() == want, name
        assert GOLDEN[name + "/inputs_sha256"].tolist() == DU.input_digest(*inputs(name)).tolist(), name      # the generator has not drifted
        assert cs["p"] <= 300


@pytest.mark.parametrize("name", NAMES)
def test_decode_equals_reference(name):
    cs = DU.GOLDEN_CASES[name]
    boxes, _ = DU.boxes_scores(cs, *inputs(name))
    if cs["prior"]:
        assert DU.same_bits(np.ascontiguousarray(boxes, np.float32), GOLDEN[name + "/boxes"])


@pytest.mark.parametrize("style", ["closed", "stable"])
@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_reference(name, style):
    """rows, order and bits; "closed" is the order the kernels implement: score descending, label ascending, index ascending"""
    cs = DU.GOLDEN_CASES[name]
    boxes, sc = DU.boxes_scores(cs, *inputs(name))
    rows, counts = DU.detect(boxes, sc, cs, style=style)
    assert DU.same_bits(rows, GOLDEN[name + "/rows"])
    assert sum(counts) == len(rows) and all(k <= cs["keep"] for k in counts)


def test_output_block_layout():
    for name in ("keeps_nothing", "one_image_empty", "all_rows_filled"):
        cs = DU.GOLDEN_CASES[name]
        y, count = DU.detout_ref(cs, *inputs(name))
        rows = GOLDEN[name + "/rows"]
        assert y.shape == (cs["n"] * cs["keep"], 7) and count.shape == (1 + cs["n"],) and count.dtype == np.int32
        assert count[0] == len(rows) == count[1:].sum()
        assert DU.same_bits(y[:len(rows)], rows) and (y[len(rows):] == -1).all()
    assert DU.detout_ref(DU.GOLDEN_CASES["keeps_nothing"], *inputs("keeps_nothing"))[1].tolist() == [0, 0, 0]
    assert DU.detout_ref(DU.GOLDEN_CASES["one_image_empty"], *inputs("one_image_empty"))[1][2] == 0
    cs = DU.GOLDEN_CASES["all_rows_filled"]
    assert DU.detout_ref(cs, *inputs("all_rows_filled"))[1].tolist() == [cs["n"] * cs["keep"]] + [cs["keep"]] * cs["n"]


@pytest.mark.parametrize("name", [n for n in NAMES if DU.GOLDEN_CASES[n]["code"] == DU.CENTER_SIZE])
def test_center_size_margin(name):
    """a last-bit difference in a decoded CENTER_SIZE box must not flip an NMS decision: every compared overlap is further than 1e-3 from
    the threshold in force"""
    m = DU.nms_margin(DU.GOLDEN_CASES[name], *inputs(name))
    print(name, "margin", m)
    assert m > 1e-3


def test_cases_reach_what_they_are_for():
    ov = []
    cs = DU.GOLDEN_CASES["exact_thresh"]
    b, s = DU.boxes_scores(cs, *inputs("exact_thresh"))
    DU.detect(b, s, cs, overlaps=ov)
    assert any(o == t for o, t in ov), "no overlap exactly equal to the threshold"
    ov = []
    cs = DU.GOLDEN_CASES["zero_area"]
    b, s = DU.boxes_scores(cs, *inputs("zero_area"))
    DU.detect(b, s, cs, overlaps=ov)
    assert any(np.isnan(o) for o, _ in ov), "no 0 / 0 overlap"
    cs = DU.GOLDEN_CASES["inverted"]
    b, _ = DU.boxes_scores(cs, *inputs("inverted"))
    assert (b[..., 2] < b[..., 0]).any()
    ov = []
    cs = DU.GOLDEN_CASES["eta"]
    b, s = DU.boxes_scores(cs, *inputs("eta"))
    DU.detect(b, s, cs, overlaps=ov)
    assert len({t for _, t in ov}) > 2, "the adaptive threshold never moved"


@pytest.mark.parametrize("defect", DU.DEFECTS)
def test_injected_defect_changes_some_case(defect):
    changed = []
    for name in NAMES:
        cs = DU.GOLDEN_CASES[name]
        good_y, good_c = DU.detout_ref(cs, *inputs(name))
        dirty = np.full_like(good_y, 7.0)
        y, c = DU.detout_ref(cs, *inputs(name), defect=defect, y_before=dirty)
        if not (DU.same_bits(y, good_y) and DU.same_bits(c, good_c)):
            changed.append(name)
    print(defect, "->", changed)
    assert changed


# ---- descriptor validation (create needs no device) ----
def _desc(**kw):
    from anakin_amd import lib as L
    d = L.DetoutDesc()
    d.n, d.classes, d.priors, d.code_type, d.variance_in_target, d.has_prior = 2, 3, 16, 1, 0, 1
    d.share_location, d.background_id, d.keep_top_k, d.nms_top_k = 1, 0, 10, 20
    d.conf_thresh, d.nms_thresh, d.nms_eta, d.dtype = 0.3, 0.45, 1.0, L.F32
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _create(d):
    from anakin_amd import lib as L
    lib = L.load()
    h = C.c_void_p()
    rc = lib.saber_hip_detout_create(C.byref(d), C.byref(h))
    err = lib.saber_hip_last_error().decode()
    return rc, err, h


REFUSED = [
    (dict(dtype=1), "UNIMPL", "FP32 only"),
    (dict(share_location=0), "UNIMPL", "share_location"),
    (dict(keep_top_k=0), "UNIMPL", "keep_top_k"),
    (dict(keep_top_k=-1), "UNIMPL", "keep_top_k"),
    (dict(nms_top_k=0), "UNIMPL", "nms_top_k"),
    (dict(nms_top_k=-1), "UNIMPL", "nms_top_k"),
    (dict(nms_top_k=1025), "UNIMPL", "nms_top_k"),
    (dict(classes=400, keep_top_k=5000, nms_top_k=1024, priors=2000), "UNIMPL", "keep_top_k"),
    (dict(n=0), "INVALID", "non-positive"),
    (dict(priors=0), "INVALID", "non-positive"),
    (dict(classes=0), "INVALID", "non-positive"),
    (dict(code_type=0), "INVALID", "code_type"),
    (dict(code_type=4), "INVALID", "code_type"),
    (dict(background_id=3), "INVALID", "background_id"),
    (dict(nms_eta=0.0), "INVALID", "nms_eta"),
    (dict(nms_eta=1.5), "INVALID", "nms_eta"),
]


@pytest.mark.parametrize("kw,status,text", REFUSED, ids=[",".join("%s=%s" % kv for kv in r[0].items()) for r in REFUSED])
def test_refused_descriptor(kw, status, text):
    from anakin_amd import lib as L
    rc, err, h = _create(_desc(**kw))
    assert rc == (L.UNIMPL if status == "UNIMPL" else INVALID_VALUE), err
    assert text in err and err.startswith("detout:"), err
    assert not h.value


def test_accepted_descriptor_and_forms():
    from anakin_amd import lib as L
    lib = L.load()
    rc, err, h = _create(_desc())
    assert rc == 0, err
    assert lib.saber_hip_detout_out_rows(h) == 20
    assert lib.saber_hip_detout_algo(h).decode() in ("detout_direct_f32", "detout_mask_f32")
    for f in (1, 0):
        assert lib.saber_hip_detout_set_tile(h, f) == 0 and lib.saber_hip_detout_get_tile(h) == f
    assert lib.saber_hip_detout_set_tile(h, 2) == INVALID_VALUE and lib.saber_hip_detout_get_tile(h) == 0
    lib.saber_hip_detout_destroy(h)
    rc, err, h = _create(_desc(nms_eta=0.5))      # eta < 1: form 1 must refuse
    assert rc == 0, err
    assert lib.saber_hip_detout_algo(h).decode() == "detout_direct_f32"
    assert lib.saber_hip_detout_set_tile(h, 1) == INVALID_VALUE and "eta" in lib.saber_hip_last_error().decode()
    assert lib.saber_hip_detout_get_tile(h) == 0
    lib.saber_hip_detout_destroy(h)
    rc, err, h = _create(_desc(keep_top_k=5000, nms_top_k=1024, classes=3, priors=2000))      # keep_top_k >= every possible total: no cut, accepted
    assert rc == 0, err
    lib.saber_hip_detout_destroy(h)


# ---- the cases past one mask word, 256 kept boxes, one sort and 256 classes (DU.SCALE_CASES): each reaches what it is named for --------------
SCALE = DU.scale_names()
_SC = {}


def scale(name):
    """a scale case, its inputs, the per-class lists and the restatement's output: computed once"""
    if name not in _SC:
        cs = DU.scale_case(name)
        ins = DU.scale_inputs(name)
        boxes, sc = DU.boxes_scores(cs, *ins)
        memo = {}
        y, count = DU.detout_ref(cs, *ins, nms_memo=memo)
        _SC[name] = dict(cs=cs, ins=ins, boxes=boxes, sc=sc, memo=memo, y=y, count=count)
    return _SC[name]


def well_formed(cs, y, count, sorted_lists=True):
    n, keep = cs["n"], cs["keep"]
    assert y.shape == (n * keep, 7) and y.dtype == np.float32 and count.shape == (1 + n,) and count.dtype == np.int32
    assert count[0] == count[1:].sum() and (count[1:] <= keep).all() and (count[1:] >= 0).all()
    assert (y[count[0]:] == -1).all()
    rows = y[:count[0]]
    assert rows[:, 0].tolist() == [i for i in range(n) for _ in range(count[1 + i])]      # image after image
    assert ((rows[:, 1] >= 0) & (rows[:, 1] < cs["c"]) & (rows[:, 1] != cs["bg"])).all()
    assert (rows[:, 2] > np.float32(cs["conf_t"])).all()
    for i in range(n):      # inside an image the labels ascend, inside a label the scores descend
        r = rows[rows[:, 0] == i]
        assert (np.diff(r[:, 1]) >= 0).all() and (not sorted_lists or ((np.diff(r[:, 2]) <= 0) | (np.diff(r[:, 1]) > 0)).all())


def entries(s, n):
    """every (class, prior index, score) image n keeps before the keep_top_k cut"""
    return [(c, i, float(s["sc"][n, c, i])) for c in range(s["cs"]["c"]) if (n, c, None) in s["memo"] for i in s["memo"][(n, c, None)]]


def cut_tie(s, n):
    """the entries of image n that share the score at its keep_top_k cut: (score, the classes of those selected, the classes of those cut off)"""
    cs = s["cs"]
    allv = entries(s, n)
    assert len(allv) > cs["keep"] == s["count"][1 + n]
    first = int(s["count"][1:1 + n].sum())
    rows = s["y"][first:first + cs["keep"]]
    at = float(rows[:, 2].min())
    inside = [int(c) for c in rows[rows[:, 2] == np.float32(at), 1]]
    every = sorted(c for c, _, v in allv if v == at)
    outside = list(every)
    for c in inside:
        outside.remove(c)
    return at, inside, outside


@pytest.mark.parametrize("name", SCALE)
def test_scale_case_is_well_formed_and_both_cut_orders_agree(name):
    """equal scores across classes are common in these cases: the reference's stable sort and the closed-form order give the same bytes"""
    s = scale(name)
    well_formed(s["cs"], s["y"], s["count"])
    y, count = DU.detout_ref(s["cs"], *s["ins"], style="stable", nms_memo=s["memo"])
    assert DU.same_bits(y, s["y"]) and DU.same_bits(count, s["count"])
    from anakin_amd import lib as L
    d = _desc(n=s["cs"]["n"], classes=s["cs"]["c"], priors=s["cs"]["p"], keep_top_k=s["cs"]["keep"], nms_top_k=s["cs"]["nms_k"], background_id=s["cs"]["bg"],
              nms_eta=s["cs"]["eta"], code_type=s["cs"]["code"])
    rc, err, h = _create(d)      # the op accepts the descriptor
    assert rc == 0, err
    L.load().saber_hip_detout_destroy(h)


def dense_traces(name):
    s = scale(name)
    return [DU.nms_trace(s["boxes"][0], s["sc"][0, c], s["cs"]) for c in range(s["cs"]["c"])]


@pytest.mark.parametrize("k", DU.DENSE_K)
def test_dense_cases_suppress_across_mask_words(k):
    """A. a suppressed candidate whose every suppressor sits in another 64-bit word is one a word-local kernel would keep"""
    tr = dense_traces("dense_k%d" % k)
    for c, (m, kept, by) in enumerate(tr):
        assert m == k      # the list is full: (k + 63) / 64 words
        cross = [j for j, sup in by.items() if all(i // 64 != j // 64 for i in sup)]
        last = [j for j in cross if j // 64 == (m - 1) // 64]
        print("nms_top_k %d class %d: %d words, %d kept (last at %d), %d suppressed only from another word, %d of them in the last word"
              % (k, c, (m + 63) // 64, len(kept), kept[-1], len(cross), len(last)))
        if k == 64:
            assert not cross
        if k >= 128 and k % 64 != 1:
            assert last
        if k == 1024:
            assert len(cross) > 700 and kept[-1] >= 1015
    if k % 64 == 1:      # one candidate alone in the last word: kept in one class; in the other suppressed, from another word of course
        alone = sorted((k - 1) in kept for _, kept, _ in tr)
        assert alone == [False, True]
        assert all(all(i // 64 != (k - 1) // 64 for i in by[k - 1]) for _, kept, by in tr if (k - 1) not in kept)


def test_more_than_256_kept_boxes_suppress():
    """B. candidates that fail only against kept boxes behind the first 256: the second turn of the direct form's strided vote"""
    m, kept, by = dense_traces("kept_past_256")[0]
    rank = {p: r for r, p in enumerate(kept)}
    late = [j for j, sup in by.items() if all(rank[i] >= 256 for i in sup)]
    print("%d candidates, %d kept, %d suppressed only by kept boxes behind the first 256" % (m, len(kept), len(late)))
    assert m == 1024 and len(kept) > 256 and len(late) >= 50


def candidates(s, c):
    with np.errstate(all="ignore"):
        return s["sc"][0, c] > np.float32(s["cs"]["conf_t"])


def test_selection_cases_cross_the_sorts():
    """C. disjoint boxes: nothing is suppressed, the rows are the selection. The number of sorts is select_top's schedule (DU.sorts_of)"""
    for name in [n for n in DU.SCALE_CASES if n.startswith("sel_")]:
        s = scale(name)
        cs = s["cs"]
        for c in range(cs["c"]):
            cand = candidates(s, c)
            assert s["memo"][(0, c, None)] == np.nonzero(cand)[0][np.argsort(-s["sc"][0, c][cand], kind="stable")][:cs["nms_k"]].tolist()      # nothing suppressed
            print(name, "class", c, int(cand.sum()), "candidates, (sorts, sorts onto a full running top):", DU.sorts_of(cand, cs["nms_k"]))
    s = scale("sel_ties_9000")      # C1: the score at the cut is held on both sides of two sorts, and by losers
    for c in range(2):
        sc, kept = s["sc"][0, c], s["memo"][(0, c, None)]
        assert candidates(s, c).all() and len(kept) == 1024
        tied = np.nonzero(sc == sc[kept[-1]])[0]
        print("sel_ties_9000 class %d: %d priors at the cut's score %g, the last selected is index %d" % (c, len(tied), sc[kept[-1]], kept[-1]))
        assert tied.min() < 3072 and tied.max() > 8192 and tied.max() > kept[-1] and int((sc >= sc[kept[-1]]).sum()) > 1024
        assert DU.sorts_of(candidates(s, c), 1024) == (3, 2)
    for p in DU.SEAM_P:      # C2: the leaders are the last items of a sort and the first of the next
        s = scale("sel_seam_%d" % p)
        at = sorted({i for i in (p - 1, DU.SORT_CAP - 1, DU.SORT_CAP) if i < p})
        orders = set()
        for c in range(2):
            sc = s["sc"][0, c]
            assert candidates(s, c).all() and len(np.unique(sc)) == p
            lead = s["memo"][(0, c, None)][:len(at)]
            assert sorted(lead) == at
            orders.add(tuple(lead))
        assert len(orders) == 2 or len(at) == 1
    s = scale("sel_sparse_20000")      # C3: a sparse fill, a full running top carried over several sorts
    for c in range(2):
        cand = candidates(s, c)
        assert 0.25 < cand.mean() < 0.35 and len(np.unique(s["sc"][0, c])) == 20000
        sorts, full = DU.sorts_of(cand, 1024)
        assert sorts >= 3 and full >= 2
    s = scale("sel_exact_cap_6000")
    for c in range(2):
        assert int(candidates(s, c).sum()) == DU.SORT_CAP and DU.sorts_of(candidates(s, c), 1024)[0] >= 2
    s = scale("sel_tail_12000")      # C4
    for c in range(2):
        cand = candidates(s, c)
        assert not cand[:2 * DU.SORT_CAP].any() and 200 < cand.sum() < 1024 and s["count"][0] == cand.sum() + candidates(s, 1 - c).sum()
    s = scale("sel_last_only_12000")
    for c in range(2):
        assert np.nonzero(candidates(s, c))[0].tolist() == [11999]
    assert s["count"].tolist() == [2, 2]


@pytest.mark.parametrize("c", DU.CLASSES + (1100,))
def test_class_cases_pass_one_block_of_classes(c):
    """D. with the cut: rows of classes >= 256, and the cut's score held by a selected class below 256 and by a class >= 256 that is cut off"""
    s = scale("cls_%d_cut" % c)
    cs = s["cs"]
    assert cs["keep"] == 40 and s["count"].tolist() == [80, 40, 40]
    for n in range(2):
        at, inside, outside = cut_tie(s, n)
        labels = s["y"][40 * n:40 * n + 40, 1]
        print("classes %d image %d: %d rows of classes >= 256; at the cut's score %g: selected classes %d .. %d, cut off %d entries up to class %d"
              % (c, n, int((labels >= 256).sum()), at, min(inside), max(inside), len(outside), max(outside)))
        if c > 256:
            assert (labels >= 256).any() and min(inside) < 256 and max(outside) >= 256
        assert outside and max(inside) <= min(outside)
    if c == 1100:      # the per-image selection runs over C * K > SORT_CAP entries: more than one sort, with ties
        for n in range(2):
            flags = np.array([j < len(s["memo"].get((n, cc, None), ())) for cc in range(c) for j in range(cs["nms_k"])])
            assert len(flags) > DU.SORT_CAP and DU.sorts_of(flags, cs["keep"])[0] >= 2
    else:
        full = scale("cls_%d_all" % c)
        assert full["cs"]["keep"] == c * 4 and (full["count"][1:] < c * 4).all() and (full["count"][1:] > 40).all()
        if c > 256:
            assert (full["y"][:full["count"][0], 1] >= 256).any()
        assert DU.same_bits(full["ins"][1], s["ins"][1])


@pytest.mark.parametrize("keep", DU.CUT_KEEP)
def test_cut_over_five_full_classes_with_ties(keep):
    """E. 5 x 1024 kept entries in eight score levels: the tie at the cut spans classes"""
    s = scale("cut_ties_keep%d" % keep)
    assert len(entries(s, 0)) == 5 * 1024 and len({v for _, _, v in entries(s, 0)}) == 8
    at, inside, outside = cut_tie(s, 0)
    print("keep_top_k %d: at the cut's score %g %d selected (classes %s), %d cut off (classes %s); sorts %s"
          % (keep, at, len(inside), sorted(set(inside)), len(outside), sorted(set(outside)), DU.sorts_of(np.ones(5 * 1024, bool), keep)))
    assert inside and outside and len(set(inside) | set(outside)) >= 2
    assert DU.sorts_of(np.ones(5 * 1024, bool), keep)[0] == 2


def test_batch_and_degenerate_cases():
    """F. seventeen images, two of them empty, some over keep_top_k and some under it; a lone background class; one prior"""
    s = scale("batch_17")
    cs, count = s["cs"], s["count"]
    print("batch_17 counts", count.tolist())
    assert cs["n"] == 17 and count[1 + 3] == 0 == count[1 + 9] and 0 < count[0] < 17 * cs["keep"]
    assert any(len(entries(s, n)) > cs["keep"] for n in range(17)) and any(0 < len(entries(s, n)) < cs["keep"] for n in range(17))
    s = scale("all_background")
    assert s["count"].tolist() == [0, 0, 0] and (s["y"] == -1).all()
    s = scale("one_prior")
    assert s["count"].tolist() == [1, 1] and (s["y"][1:] == -1).all()


def test_sweep_list():
    """G. the fixed seed list: every CENTER_SIZE entry passes the margin condition, a quarter of the list is CENTER_SIZE behind priors, a
    quarter follows the adaptive threshold"""
    cases = [DU.scale_case("sweep_%d" % seed) for seed in DU.SWEEP_SEEDS]
    assert len(cases) == 48 == len(set(DU.SWEEP_SEEDS))
    center = 0
    for seed, cs in zip(DU.SWEEP_SEEDS, cases):
        assert 1 <= cs["n"] <= 4 and 1 <= cs["c"] <= 6 and 1 <= cs["p"] <= 200 and -1 <= cs["bg"] < cs["c"] and 1 <= cs["keep"] <= 60
        assert 1 <= cs["nms_k"] <= 120 and 0 <= cs["conf_t"] <= 0.6 and 0.2 <= cs["nms_t"] <= 0.7 and (cs["eta"] == 1 or 0.6 <= cs["eta"] <= 0.95)
        if cs["code"] == DU.CENTER_SIZE:
            m = DU.nms_margin(cs, *DU.scale_inputs("sweep_%d" % seed))
            print("sweep_%d margin %g" % (seed, m))
            assert m > 1e-3
            center += cs["prior"]
    assert center >= 12 and sum(cs["eta"] < 1 for cs in cases) >= 12
    assert {cs["code"] for cs in cases} == {1, 2, 3} and {(cs["vit"], cs["prior"]) for cs in cases} == {(a, b) for a in (False, True) for b in (False, True)}
    assert any(cs["bg"] == -1 for cs in cases) and any(cs["bg"] == cs["c"] - 1 for cs in cases)


# the defects of DU.SCALE_DEFECTS, and the cases each of them must change. chunk_ties: with keep_top_k = 1 the leader of the first block IS the
# leader (class 0 holds the top score level), so of E the two deep cuts show it
MUST_CHANGE = {
    "word_local": ["dense_k%d" % k for k in DU.DENSE_K if k > 64],
    "vote_256": ["kept_past_256"],
    "first_block": [n for n in DU.SCALE_CASES if n.startswith("sel_") and DU.SCALE_CASES[n]["p"] > DU.SORT_CAP],
    "chunk_ties": ["sel_ties_9000", "cut_ties_keep3000", "cut_ties_keep3072"],
    "classes_256": [n for n in DU.SCALE_CASES if n.startswith("cls_") and DU.SCALE_CASES[n]["c"] > 256],
}


@pytest.mark.parametrize("defect,name", [(d, n) for d in DU.SCALE_DEFECTS for n in MUST_CHANGE[d]])
def test_scale_defect_changes_its_cases(defect, name):
    s = scale(name)
    y, count = DU.detout_ref(s["cs"], *s["ins"], defect=defect, nms_memo=s["memo"])
    well_formed(s["cs"], y, count, sorted_lists=defect != "chunk_ties")      # (that one concatenates sorted blocks)
    assert not (DU.same_bits(y, s["y"]) and DU.same_bits(count, s["count"]))


def test_scale_defects_are_covered():
    assert sorted(MUST_CHANGE) == sorted(DU.SCALE_DEFECTS) and all(MUST_CHANGE.values())
    assert len(MUST_CHANGE["first_block"]) == 8 and len(MUST_CHANGE["classes_256"]) == 7 and len(MUST_CHANGE["word_local"]) == 5
