"""DetectionOutput without a GPU: the numpy restatement (tests/detout_util.py) against outputs recorded from the reference's own code
(tests/golden/detout_ref.npz, scripts/record_detout_golden.py), the closed-form keep_top_k order, the margin condition of the
CENTER_SIZE cases, descriptor validation, and proof that each injected defect is visible in some case."""
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
