"""DetectionOutput expected values: a numpy float32 restatement of the reference's decode_bbox_* (saber/funcs/impl/x86/detection_helper.cpp),
get_max_score_index / jaccard_overlap / apply_nms_fast / nms_detect (saber/funcs/impl/detection_helper.cpp) and the x86 dispatch's packing
(saber_detection_output.cpp). tests/test_detout_cpu.py asserts it == outputs recorded from that code (tests/golden/detout_ref.npz,
scripts/record_detout_golden.py); the GPU tests compare the kernels against it.

Every product, sum and quotient is a float32 operation; the one transcendental, CENTER_SIZE's `exp`, is expf (see expf below)."""
import zlib

import numpy as np

CORNER, CENTER_SIZE, CORNER_SIZE = 1, 2, 3      # CodeType (saber/saber_types.h)
SORT_CAP = 4096      # keys one workgroup sorts at a time (detout.hip DETOUT_SORT_CAP), both forms
f32 = np.float32

DEFECTS = ("ge_thresh", "unstable", "lt_nms", "nan_kept", "no_eta", "cut_by_index", "pad_left")
# defects only a case past one mask word, 256 kept boxes, one sort chunk or 256 classes shows (SCALE_CASES, SCALE_DEFECTS below)
PACK_DEFECTS = ("cut_by_index", "pad_left", "classes_256")      # these leave the per-class lists alone


def case(n, c, p, code=CORNER, vit=False, prior=True, bg=0, keep=20, nms_k=50, conf_t=0.3, nms_t=0.45, eta=1.0, special=None):
    return dict(n=n, c=c, p=p, code=code, vit=vit, prior=prior, bg=bg, keep=keep, nms_k=nms_k, conf_t=conf_t, nms_t=nms_t, eta=eta, special=special)


# the recorded cases (P <= 300 each); CENTER_SIZE cases carry the margin condition (nms_margin below), CORNER cases the adversarial inputs
GOLDEN_CASES = {
    "corner": case(2, 3, 40),
    "corner_vit": case(1, 4, 33, vit=True, bg=1),
    "center": case(2, 3, 60, code=CENTER_SIZE),
    "center_vit": case(1, 5, 47, code=CENTER_SIZE, vit=True, bg=2, keep=9),
    "center_300": case(3, 4, 300, code=CENTER_SIZE, keep=40, nms_k=100, conf_t=0.8),
    "csize": case(2, 3, 50, code=CORNER_SIZE),
    "csize_vit": case(1, 3, 29, code=CORNER_SIZE, vit=True, bg=-1),
    "noprior": case(2, 4, 45, prior=False, bg=3),
    "noprior_bgm1": case(1, 2, 64, prior=False, bg=-1, keep=7),
    "bg_middle": case(2, 5, 37, bg=2, keep=12),
    "ties_nms_cut": case(2, 3, 48, special="ties", nms_k=7, keep=30, conf_t=0.25),      # scores equal to the threshold too
    "ties_keep_cut": case(2, 4, 40, special="ties", nms_k=30, keep=5, conf_t=0.2, bg=-1),
    "exact_thresh": case(1, 3, 36, prior=False, special="exact", nms_t=0.5, conf_t=0.05, keep=40),
    "zero_area": case(2, 3, 30, prior=False, special="zero", conf_t=0.1, keep=40),
    "inverted": case(2, 3, 40, special="inverted", conf_t=0.1, keep=40),
    "nan_inf_scores": case(2, 3, 40, special="nanscore", conf_t=0.1),
    "eta": case(2, 3, 80, eta=0.8, nms_t=0.9, conf_t=0.1, keep=60, nms_k=80),
    "eta_noprior": case(1, 2, 120, prior=False, eta=0.7, nms_t=0.95, conf_t=0.05, keep=200, nms_k=120, bg=-1),
    "keeps_nothing": case(2, 3, 20, conf_t=2.0),
    "one_image_empty": case(3, 3, 24, special="img1_empty", conf_t=0.4),
    "more_than_nms_k": case(1, 3, 100, nms_k=10, conf_t=0.01, keep=50),
    "fewer_than_nms_k": case(1, 3, 16, nms_k=400, conf_t=0.6, keep=50),
    "all_rows_filled": case(3, 4, 60, prior=False, special="disjoint", keep=6, conf_t=0.0, nms_k=60),
    "at_thresh": case(1, 3, 24, special="ties", conf_t=0.25, nms_k=50, keep=80),      # scores exactly equal to conf_thresh
    "p8": case(1, 2, 8, keep=1, nms_k=1, conf_t=0.0),
}


# CENTER_SIZE cases: seeds for which every compared overlap is further than 1e-3 from the threshold in force (test_center_size_margin)
SEEDS = {"center": 7, "center_vit": 1, "center_300": 116}


def seed_of(name):
    return SEEDS.get(name, zlib.crc32(name.encode()) & 0x7fffffff)


def make(cs, rng):
    """-> loc [N, P*4], conf ([N, P, C] with priors, else [N, C, P]), prior ([2, P*4] or None), all float32"""
    n, c, p, sp = cs["n"], cs["c"], cs["p"], cs["special"]
    g = max(2, p // 6)
    centres = rng.uniform(0.2, 0.8, (g, 2))
    which = rng.integers(0, g, p)
    ctr = centres[which] + rng.normal(0, 0.03, (p, 2))
    half = rng.uniform(0.05, 0.15, (p, 2))
    boxes = np.concatenate([ctr - half, ctr + half], 1).astype(f32)      # [P, 4]
    conf = rng.random((n, p, c)).astype(f32)
    if sp == "ties":
        conf = (np.floor(conf * 4) / 4).astype(f32)
    if sp == "nanscore":
        m = rng.integers(0, 12, conf.shape)
        conf[m == 0] = np.nan
        conf[m == 1] = np.inf
        conf[m == 2] = -np.inf
        conf[m == 3] = -0.0
    if sp == "img1_empty":
        conf[1] = f32(0.25) * conf[1]
    if sp == "exact":      # x extents 2, 1, 4 from one corner: overlaps 1/2 (== the threshold), 1/4, 1/2; cells far apart; every value a multiple of 1/64
        b = np.zeros((p, 4), f32)
        for i in range(p):
            o, w = 8 * (i // 3 % 4), (2, 1, 4)[i % 3]
            r = i // 12
            b[i] = np.array([o, 2 * r, o + w, 2 * r + 1], f32) / f32(64)
        boxes = b
    if sp == "zero":       # pairs of identical zero-area boxes (0 / 0) between ordinary ones
        for i in range(0, p - 1, 3):
            boxes[i, 2:] = boxes[i, :2]
            boxes[i + 1] = boxes[i]
    if sp == "disjoint":   # no two boxes touch: nothing is suppressed, every image keeps more than keep_top_k
        for i in range(p):
            boxes[i] = np.array([i, 0, i + 0.5, 1], f32) / f32(128)
    if cs["prior"]:
        if cs["code"] == CENTER_SIZE:
            loc = rng.normal(0, 0.6, (n, p, 4)).astype(f32)
        else:
            loc = rng.normal(0, 0.2 if not cs["vit"] else 0.03, (n, p, 4)).astype(f32)
        if sp == "inverted":
            loc[:, ::4, 2] -= f32(3.0)      # xmax far left of xmin once decoded
        var = np.tile(np.array([0.1, 0.1, 0.2, 0.2], f32), p)
        prior = np.stack([boxes.reshape(-1), var]).astype(f32)
        return loc.reshape(n, p * 4), conf, prior
    loc = np.repeat(boxes[None], n, 0)
    if sp not in ("exact", "disjoint"):
        loc = (loc + rng.normal(0, 0.01, loc.shape)).astype(f32)
        if sp == "zero":
            loc[:] = boxes[None]
    return np.ascontiguousarray(loc.reshape(n, p * 4), f32), np.ascontiguousarray(conf.transpose(0, 2, 1)), None


def inputs(name):
    """the inputs of a recorded case: regenerated, not stored - the fixture pins them by digest (input_digest)"""
    return make(GOLDEN_CASES[name], np.random.default_rng(seed_of(name)))


def input_digest(loc, conf, prior):
    import hashlib
    h = hashlib.sha256()
    for a in (loc, conf, prior):
        h.update(b"-" if a is None else np.ascontiguousarray(a).tobytes())
    return np.frombuffer(h.digest(), np.uint8).copy()


def expf(x):
    """the reference's `exp` on a float resolves to the float overload (glibc expf, whose error stays below 0.51 ulp): the double
    exponential rounded to float32 once - test_decode_equals_reference holds this against the recording"""
    return np.exp(x.astype(np.float64)).astype(f32)


def decode(loc, prior, code, vit):
    """the six decode_bbox_* functions -> [N, P, 4] float32"""
    n = loc.shape[0]
    l = loc.reshape(n, -1, 4).astype(f32)
    pr = prior[0].reshape(-1, 4).astype(f32)[None]
    v = prior[1].reshape(-1, 4).astype(f32)[None]
    with np.errstate(all="ignore"):
        if code == CORNER:
            return (pr + l).astype(f32) if vit else (pr + (l * v).astype(f32)).astype(f32)
        pw = (pr[..., 2] - pr[..., 0]).astype(f32)
        ph = (pr[..., 3] - pr[..., 1]).astype(f32)
        psz = np.stack([pw, ph, pw, ph], -1)
        if code == CORNER_SIZE:
            t = l if vit else (l * v).astype(f32)
            return (pr + (t * psz).astype(f32)).astype(f32)
        assert code == CENTER_SIZE
        pcx = ((pr[..., 0] + pr[..., 2]).astype(f32) / f32(2)).astype(f32)
        pcy = ((pr[..., 1] + pr[..., 3]).astype(f32) / f32(2)).astype(f32)
        if vit:
            tx, ty, tw, th = l[..., 0], l[..., 1], l[..., 2], l[..., 3]
        else:
            tx, ty = (v[..., 0] * l[..., 0]).astype(f32), (v[..., 1] * l[..., 1]).astype(f32)
            tw, th = (v[..., 2] * l[..., 2]).astype(f32), (v[..., 3] * l[..., 3]).astype(f32)
        cx = ((tx * pw).astype(f32) + pcx).astype(f32)
        cy = ((ty * ph).astype(f32) + pcy).astype(f32)
        w = (expf(tw) * pw).astype(f32)
        h = (expf(th) * ph).astype(f32)
        hw, hh = (w / f32(2)).astype(f32), (h / f32(2)).astype(f32)
        return np.stack([(cx - hw).astype(f32), (cy - hh).astype(f32), (cx + hw).astype(f32), (cy + hh).astype(f32)], -1)


def jaccard_many(b1, k4):
    """jaccard_overlap(bbox1 = b1, bbox2 = each row of k4) in float32, element by element what the reference computes: std::max(a, b) is
    (a < b) ? b : a, std::min(a, b) is (b < a) ? b : a; bbox_size is 0 for an inverted box; the early-out's strict comparisons"""
    with np.errstate(all="ignore"):
        k4 = np.asarray(k4, f32).reshape(-1, 4)
        b1 = np.asarray(b1, f32)
        apart = (k4[:, 0] > b1[2]) | (k4[:, 2] < b1[0]) | (k4[:, 1] > b1[3]) | (k4[:, 3] < b1[1])
        xmin = np.where(b1[0] < k4[:, 0], k4[:, 0], b1[0])
        ymin = np.where(b1[1] < k4[:, 1], k4[:, 1], b1[1])
        xmax = np.where(k4[:, 2] < b1[2], k4[:, 2], b1[2])
        ymax = np.where(k4[:, 3] < b1[3], k4[:, 3], b1[3])
        inter = ((xmax - xmin).astype(f32) * (ymax - ymin).astype(f32)).astype(f32)
        s1 = f32(0) if (b1[2] < b1[0] or b1[3] < b1[1]) else f32(f32(b1[2] - b1[0]) * f32(b1[3] - b1[1]))
        s2 = np.where((k4[:, 2] < k4[:, 0]) | (k4[:, 3] < k4[:, 1]), f32(0), ((k4[:, 2] - k4[:, 0]).astype(f32) * (k4[:, 3] - k4[:, 1]).astype(f32)).astype(f32))
        ov = (inter / ((s1 + s2).astype(f32) - inter).astype(f32)).astype(f32)
        return np.where(apart, f32(0), ov).astype(f32)


def jaccard(b1, b2):
    return jaccard_many(b1, b2)[0]


def nms_class(boxes, scores, cs, defect=None, overlaps=None):
    """apply_nms_fast for one (image, class) -> kept prior indices in the order they were kept. overlaps: a list that receives every
    (overlap, threshold in force) the loop compares"""
    t = f32(cs["conf_t"])
    with np.errstate(all="ignore"):
        cand = np.nonzero(scores >= t if defect == "ge_thresh" else scores > t)[0]      # a NaN is no candidate
        if defect == "first_block":
            cand = cand[cand < SORT_CAP]
        neg = -(scores[cand] + f32(0))      # (-0 and +0 are one score)
    if defect == "unstable":
        cand = cand[np.lexsort((-cand, neg))]
    elif defect == "chunk_ties":      # every block of SORT_CAP indices sorted and cut on its own, the blocks one after the other
        parts = [cand[(cand // SORT_CAP) == b] for b in range((len(scores) + SORT_CAP - 1) // SORT_CAP)]
        parts = [q[np.argsort(-(scores[q] + f32(0)), kind="stable")][:cs["nms_k"] if cs["nms_k"] > -1 else None] for q in parts]
        cand = np.concatenate(parts) if parts else cand
    else:
        cand = cand[np.argsort(neg, kind="stable")]      # std::stable_sort: equal scores stay in index order
    if -1 < cs["nms_k"] < len(cand):
        cand = cand[:cs["nms_k"]]
    thr, eta = f32(cs["nms_t"]), f32(cs["eta"])
    kept = []
    kpos = np.zeros(len(cand), np.int64)    # their positions in the sorted candidate list
    kb = np.zeros((len(cand), 4), f32)      # the kept boxes in the order they were kept
    for pos, i in enumerate(cand.tolist()):
        ov = jaccard_many(boxes[i], kb[:len(kept)])
        with np.errstate(all="ignore"):
            ok = (ov < thr) if defect == "lt_nms" else (ov <= thr)      # a NaN overlap fails
        if defect == "nan_kept":
            ok = ok | np.isnan(ov)
        if defect == "word_local":      # a kept box reaches only the 64 sorted positions of its own block
            ok = ok | (kpos[:len(kept)] // 64 != pos // 64)
        if defect == "vote_256":        # only the first 256 kept boxes are asked
            ok[256:] = True
        keep = bool(ok.all())
        if overlaps is not None:      # the reference stops at the first failure
            last = len(ov) if keep else int(np.argmin(ok)) + 1
            overlaps.extend((float(o), float(thr)) for o in ov[:last])
        if keep:
            kb[len(kept)] = boxes[i]
            kpos[len(kept)] = pos
            kept.append(i)
            if defect != "no_eta" and eta < 1 and thr > 0.5:
                thr = f32(thr * eta)
    return kept


def detect(boxes, conf_cp, cs, defect=None, style="closed", overlaps=None, nms_memo=None):
    """nms_detect on decoded boxes [N, P, 4] and scores [N, C, P] -> (rows [M, 7] float32, per-image counts). style "closed": the keep_top_k
    cut by (score descending, label ascending, index ascending); "stable": the reference's stable sort of its label-ascending list.
    nms_memo: a dict a caller passes to several calls on the SAME inputs, so that the per-class lists are computed once"""
    rows, counts = [], []
    nms_defect = None if defect in PACK_DEFECTS else defect
    for n in range(cs["n"]):
        per = {}
        for c in range(cs["c"]):
            if c == cs["bg"] or (defect == "classes_256" and c >= 256):
                continue
            if nms_memo is None or overlaps is not None:
                per[c] = nms_class(boxes[n], conf_cp[n, c], cs, defect, overlaps)
            else:
                if (n, c, nms_defect) not in nms_memo:
                    nms_memo[(n, c, nms_defect)] = nms_class(boxes[n], conf_cp[n, c], cs, nms_defect)
                per[c] = nms_memo[(n, c, nms_defect)]
        flat = [(c, i) for c in sorted(per) for i in per[c]]
        if cs["keep"] > -1 and len(flat) > cs["keep"]:
            if defect == "chunk_ties":      # the per-image cut too: blocks of SORT_CAP entries of the [class][position] table, no merge
                where = {(c, i): c * cs["nms_k"] + j for c in per for j, i in enumerate(per[c])}
                flat.sort(key=lambda ci: (where[ci] // SORT_CAP, -float(conf_cp[n, ci[0], ci[1]]), ci[0], ci[1]))
                flat = [ci for b in sorted({where[ci] // SORT_CAP for ci in flat}) for ci in [q for q in flat if where[q] // SORT_CAP == b][:cs["keep"]]]
            elif defect == "cut_by_index":
                flat.sort(key=lambda ci: (-float(conf_cp[n, ci[0], ci[1]]), ci[1]))
            elif style == "stable":
                flat.sort(key=lambda ci: -float(conf_cp[n, ci[0], ci[1]]))
            else:
                flat.sort(key=lambda ci: (-float(conf_cp[n, ci[0], ci[1]]), ci[0], ci[1]))
            flat = flat[:cs["keep"]]
            new = {}
            for c, i in flat:
                new.setdefault(c, []).append(i)
            flat = [(c, i) for c in sorted(new) for i in new[c]]
        counts.append(len(flat))
        for c, i in flat:
            rows.append(np.concatenate([np.array([n, c, conf_cp[n, c, i]], f32), boxes[n, i]]))
    return (np.stack(rows).astype(f32) if rows else np.zeros((0, 7), f32)), counts


def boxes_scores(cs, loc, conf, prior):
    """the decoded boxes [N, P, 4] and the scores as [N, C, P]"""
    if cs["prior"]:
        return decode(loc, prior, cs["code"], cs["vit"]), np.ascontiguousarray(conf.transpose(0, 2, 1))
    return loc.reshape(cs["n"], cs["p"], 4), conf


def detout_ref(cs, loc, conf, prior, defect=None, style="closed", y_before=None, nms_memo=None):
    """what saber_hip_detout_run writes: y [N * keep_top_k, 7] (the kept rows, then rows of -1) and count [1 + N] int32"""
    boxes, sc = boxes_scores(cs, loc, conf, prior)
    rows, counts = detect(boxes, sc, cs, defect, style, nms_memo=nms_memo)
    y = np.full((cs["n"] * cs["keep"], 7), -1, f32)
    if defect == "pad_left" and y_before is not None:
        y = y_before.copy()
    y[:len(rows)] = rows
    return y, np.array([len(rows)] + counts, np.int32)


def nms_margin(cs, loc, conf, prior):
    """the smallest |overlap - threshold in force| over every comparison the reference makes (inf where it makes none)"""
    boxes, sc = boxes_scores(cs, loc, conf, prior)
    ov = []
    detect(boxes, sc, cs, overlaps=ov)
    return min([abs(o - t) for o, t in ov if not np.isnan(o)] + [np.inf])


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- cases past one 64-bit mask word, 256 kept boxes, one sort of SORT_CAP keys and 256 classes ------------------------------------------------
# Not recorded: their expected values are detout_ref's, which the recorded cases tie to the reference. Each carries "gen": (generator, seed,
# further arguments); tests/test_detout_cpu.py asserts that each reaches the boundary it is named for.
STEP = 1024      # priors between two looks at the fill (detout.hip STEP)


def _scale(gen, *a, **kw):
    cs = case(*a, **kw)
    cs["gen"] = gen
    return cs


def _np(n, c, p, keep, nms_k, conf_t, nms_t=0.45, special=None, bg=-1):
    return dict(n=n, c=c, p=p, prior=False, bg=bg, keep=keep, nms_k=nms_k, conf_t=conf_t, nms_t=nms_t, special=special)


DENSE_K = (64, 65, 128, 129, 1000, 1024)
SEAM_P = (4095, 4096, 5120, 8192, 8193)
CLASSES = (256, 257, 300, 513)
CUT_KEEP = (1, 3000, 3072)
# 16 CENTER_SIZE entries with priors, each past the 1e-3 margin (nms_margin), 14 with eta < 1, 18 others: the first of each kind from seed 0 up
SWEEP_SEEDS = (1, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 20, 22, 23, 24, 26, 27, 28, 29, 30, 31, 37, 41, 42, 46, 48, 51, 53, 62, 63, 66, 76, 78, 94,
               99, 121, 124, 132, 137, 149, 160, 172, 175)

SCALE_CASES = {}
for _k in DENSE_K:       # A: clustered boxes, every 64-bit word of the mask form's matrix in use, no per-image cut
    SCALE_CASES["dense_k%d" % _k] = _scale(("make", 3), **_np(1, 2, 1500, 2 * _k, _k, 0.05))
# B: more kept boxes than the direct form has lanes, with real overlaps
SCALE_CASES["kept_past_256"] = _scale(("spread", 11), **_np(1, 1, 1500, 1024, 1024, 0.0, nms_t=0.3))
# C: disjoint boxes - the output is the selection itself
SCALE_CASES["sel_ties_9000"] = _scale(("select", 12, "levels8"), **_np(1, 2, 9000, 2048, 1024, -0.5, special="disjoint"))
for _p in SEAM_P:
    SCALE_CASES["sel_seam_%d" % _p] = _scale(("select", 13, "seam"), **_np(1, 2, _p, 6, 3, -0.5, special="disjoint"))
SCALE_CASES["sel_sparse_20000"] = _scale(("select", 14, "distinct"), **_np(1, 2, 20000, 2048, 1024, 0.7, special="disjoint"))
SCALE_CASES["sel_exact_cap_6000"] = _scale(("select", 15, "distinct"), **_np(1, 2, 6000, 2048, 1024, 1904.5 / 6001, special="disjoint"))
SCALE_CASES["sel_tail_12000"] = _scale(("select", 16, "tail"), **_np(1, 2, 12000, 2048, 1024, 0.9, special="disjoint"))
SCALE_CASES["sel_last_only_12000"] = _scale(("select", 17, "last"), **_np(1, 2, 12000, 2048, 1024, 0.9, special="disjoint"))
# D: more classes than the pack kernel has lanes
for _c in CLASSES:
    SCALE_CASES["cls_%d_cut" % _c] = _scale(("classes", 24), **_np(2, _c, 8, 40, 4, 0.25, special="ties", bg=7))
    SCALE_CASES["cls_%d_all" % _c] = _scale(("classes", 24), **_np(2, _c, 8, _c * 4, 4, 0.25, special="ties", bg=7))
# (nms_thresh 0.7: 3357 / 3369 of the first 1024 classes' 4096 entries are filled, so the per-image selection sorts before it has seen them all)
SCALE_CASES["cls_1100_cut"] = _scale(("classes", 24), **_np(2, 1100, 8, 40, 4, 0.25, nms_t=0.7, special="ties", bg=7))
# E: the per-image cut over 5 x 1024 kept entries, eight score levels
for _k in CUT_KEEP:
    SCALE_CASES["cut_ties_keep%d" % _k] = _scale(("cut_ties", 19), **_np(1, 5, 1030, _k, 1024, 0.0, special="disjoint"))
# F: batch, and the degenerate ends
SCALE_CASES["batch_17"] = _scale(("batch", 20, (3, 9), (1, 6, 16)), 17, 3, 40, keep=12)
SCALE_CASES["all_background"] = _scale(("make", 21), 2, 1, 16, bg=0, keep=5)
SCALE_CASES["one_prior"] = _scale(("make", 22), 1, 1, 1, bg=-1, keep=3, nms_k=5, conf_t=0.0)


def sweep_case(seed):
    """G: the descriptor of one entry of the random sweep"""
    r = np.random.default_rng([seed, 48])
    n, c, p = int(r.integers(1, 5)), int(r.integers(1, 7)), int(r.integers(1, 201))
    code = (CORNER, CENTER_SIZE, CORNER_SIZE)[int(r.integers(0, 3))]
    vit, prior = bool(r.integers(0, 2)), bool(r.integers(0, 2))
    bg, keep, nms_k = int(r.integers(-1, c)), int(r.integers(1, 61)), int(r.integers(1, 121))
    conf_t, nms_t = round(float(r.uniform(0, 0.6)), 3), round(float(r.uniform(0.2, 0.7)), 3)
    eta = 1.0 if r.integers(0, 4) else round(float(r.uniform(0.6, 0.95)), 3)
    return _scale(("make", seed), n, c, p, code=code, vit=vit, prior=prior, bg=bg, keep=keep, nms_k=nms_k, conf_t=conf_t, nms_t=nms_t, eta=eta)


def disjoint_boxes(p):
    """make()'s "disjoint" boxes"""
    i = np.arange(p, dtype=np.float64)
    return (np.stack([i, 0 * i, i + 0.5, 0 * i + 1], 1).astype(f32) / f32(128)).astype(f32)


def distinct_scores(rng, c, p):
    """[1, C, P]: every class a permutation of k / (P + 1), k = 1 .. P - distinct in float32 for P < 2^20"""
    return np.stack([((rng.permutation(p) + 1) / (p + 1)).astype(f32) for _ in range(c)])[None]


def scale_inputs(name):
    """-> loc, conf, prior of a SCALE_CASES entry (or of "sweep_<seed>")"""
    cs = scale_case(name)
    kind, seed = cs["gen"][:2]
    rng = np.random.default_rng(seed)
    n, c, p = cs["n"], cs["c"], cs["p"]
    if kind == "make":
        return make(cs, rng)
    if kind == "spread":
        ctr, half = rng.uniform(0.1, 0.9, (p, 2)), rng.uniform(0.012, 0.03, (p, 2))
        loc = np.concatenate([ctr - half, ctr + half], 1).astype(f32).reshape(1, p * 4)
        return np.repeat(loc, n, 0), rng.random((n, c, p)).astype(f32), None
    if kind == "select":
        loc = np.repeat(disjoint_boxes(p).reshape(1, p * 4), n, 0)
        mode = cs["gen"][2]
        if mode == "levels8":
            conf = (np.floor(rng.random((n, c, p)) * 8) / 8).astype(f32)
        else:
            conf = distinct_scores(rng, c, p)
        if mode == "seam":      # the three leaders sit at the ends of the sorts: P - 1, SORT_CAP - 1, SORT_CAP, in another order in every class
            conf = (conf * f32(0.5)).astype(f32)
            at = list(dict.fromkeys(i for i in (p - 1, SORT_CAP - 1, SORT_CAP) if i < p))
            for cc in range(c):
                for r, i in enumerate(at[cc % len(at):] + at[:cc % len(at)]):
                    conf[0, cc, i] = f32(0.99) - f32(0.01) * f32(r)
        if mode == "tail":      # no candidate among the first 2 * SORT_CAP priors
            conf[:, :, :2 * SORT_CAP] *= f32(0.25)
        if mode == "last":      # the last prior is the only candidate
            conf = (conf * f32(0.5)).astype(f32)
            conf[:, :, -1] = f32(0.95)
        return loc, np.ascontiguousarray(conf, f32), None
    if kind == "classes":       # make()'s quarter steps; 0.75 only in every 64th class, so that the cut falls among the many 0.5
        loc, conf, _ = make(cs, rng)
        cold = np.arange(c) % 64 != 0
        cold[0] = True
        conf[:, cold, :] = np.minimum(conf[:, cold, :], f32(0.5))
        return loc, conf, None
    if kind == "cut_ties":      # test_gpu_detout's _big shape: every score above the threshold, in eight levels
        loc, conf, _ = make(cs, rng)
        conf = ((np.floor(conf * 8) / 8).astype(f32) * f32(0.5) + f32(0.25)).astype(f32)
        return loc, conf, None
    assert kind == "batch"
    loc, conf, prior = make(cs, rng)
    for i in cs["gen"][2]:      # these images have every score below the threshold
        conf[i] = f32(0.25) * conf[i]
    for i in cs["gen"][3]:      # and these only a few above it: they stay under keep_top_k
        conf[i] = f32(0.33) * conf[i]
    return loc, conf, prior


def scale_case(name):
    return sweep_case(int(name[6:])) if name.startswith("sweep_") else SCALE_CASES[name]


def scale_names():
    return list(SCALE_CASES) + ["sweep_%d" % s for s in SWEEP_SEEDS]


SCALE_DEFECTS = ("word_local", "vote_256", "first_block", "chunk_ties", "classes_256")


def nms_trace(boxes, scores, cs):
    """one (image, class) with eta == 1, in positions of the sorted candidate list: (m, the kept positions in order, {suppressed position:
    the kept positions it fails against - all of them, not only the first})"""
    assert cs["eta"] == 1.0
    with np.errstate(all="ignore"):
        cand = np.nonzero(scores > f32(cs["conf_t"]))[0]
    cand = cand[np.argsort(-(scores[cand] + f32(0)), kind="stable")][:cs["nms_k"]]
    kept, by = [], {}
    for pos, i in enumerate(cand.tolist()):
        ov = jaccard_many(boxes[i], boxes[cand[kept]])
        with np.errstate(all="ignore"):
            bad = np.nonzero(~(ov <= f32(cs["nms_t"])))[0]
        if len(bad):
            by[pos] = [kept[k] for k in bad.tolist()]
        else:
            kept.append(pos)
    assert cand[kept].tolist() == nms_class(boxes, scores, cs)
    return len(cand), kept, by


def sorts_of(cand, K):
    """detout.hip's select_top over the candidate flags of item 0 .. len(cand): (how many sorts it runs, how many of them start from a
    running top of K keys)"""
    topn = f = sorts = full = 0
    for base in range(0, len(cand), STEP):
        if topn + f + STEP > SORT_CAP and f:
            sorts, full, topn, f = sorts + 1, full + (topn == K), min(topn + f, K), 0
        f += int(np.count_nonzero(cand[base:base + STEP]))
        assert topn + f <= SORT_CAP
    if f:
        sorts, full = sorts + 1, full + (topn == K)
    return sorts, full
