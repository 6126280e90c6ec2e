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
        neg = -(scores[cand] + f32(0))      # (-0 and +0 are one score)
    if defect == "unstable":
        cand = cand[np.lexsort((-cand, neg))]
    else:
        cand = cand[np.argsort(neg, kind="stable")]      # std::stable_sort: equal scores stay in index order
    if -1 < cs["nms_k"] < len(cand):
        cand = cand[:cs["nms_k"]]
    thr, eta = f32(cs["nms_t"]), f32(cs["eta"])
    kept = []
    kb = np.zeros((len(cand), 4), f32)      # the kept boxes in the order they were kept
    for i in cand.tolist():
        ov = jaccard_many(boxes[i], kb[:len(kept)])
        with np.errstate(all="ignore"):
            ok = (ov < thr) if defect == "lt_nms" else (ov <= thr)      # a NaN overlap fails
        if defect == "nan_kept":
            ok = ok | np.isnan(ov)
        keep = bool(ok.all())
        if overlaps is not None:      # the reference stops at the first failure
            last = len(ov) if keep else int(np.argmin(ok)) + 1
            overlaps.extend((float(o), float(thr)) for o in ov[:last])
        if keep:
            kb[len(kept)] = boxes[i]
            kept.append(i)
            if defect != "no_eta" and eta < 1 and thr > 0.5:
                thr = f32(thr * eta)
    return kept


def detect(boxes, conf_cp, cs, defect=None, style="closed", overlaps=None):
    """nms_detect on decoded boxes [N, P, 4] and scores [N, C, P] -> (rows [M, 7] float32, per-image counts). style "closed": the keep_top_k
    cut by (score descending, label ascending, index ascending); "stable": the reference's stable sort of its label-ascending list"""
    rows, counts = [], []
    for n in range(cs["n"]):
        per = {}
        for c in range(cs["c"]):
            if c == cs["bg"]:
                continue
            per[c] = nms_class(boxes[n], conf_cp[n, c], cs, defect, overlaps)
        flat = [(c, i) for c in sorted(per) for i in per[c]]
        if cs["keep"] > -1 and len(flat) > cs["keep"]:
            if defect == "cut_by_index":
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


def detout_ref(cs, loc, conf, prior, defect=None, style="closed", y_before=None):
    """what saber_hip_detout_run writes: y [N * keep_top_k, 7] (the kept rows, then rows of -1) and count [1 + N] int32"""
    boxes, sc = boxes_scores(cs, loc, conf, prior)
    rows, counts = detect(boxes, sc, cs, defect, style)
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
