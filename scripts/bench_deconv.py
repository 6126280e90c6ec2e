"""The deconv kernels (anakin_amd/csrc/deconv.hip) against each other and, on the k2 s2 rows, against the same arithmetic through the
existing FP32 1x1 conv C -> 4K (it moves the same bytes: the bar a deconv kernel of its own has to justify itself against).

  python scripts/bench_deconv.py shapes [--out DIR]   every row x batch, every form the op accepts -> DIR/shapes.json
  python scripts/bench_deconv.py table  [--out DIR]   DIR/shapes.json -> DIR/README.md (no GPU needed); exit status 1 when the static rule
                                                      (what saber_hip_deconv2d_create selects) does not hold on a row
  python scripts/bench_deconv.py check  [--out DIR]   every row x batch once per accepted form, nothing timed: each output against the float64
                                                      rule of tests/deconv_util.py (computed on the CPU) on the project's two 1e-4 criteria, forms
                                                      1 and 2 byte for byte -> DIR/check.txt; exit status 1 when a line fails

The protocol is scripts/bench_group.py's: ONE process, the forms alternating, after a warm-up, with device events:
  cold  one launch per window with the operands cold in L2 - between two timed launches a 64 MB buffer is streamed through the L2s, as the
        autotuner's ColdBench does - median of REPS windows per form;
  warm  WARM_LAUNCHES back-to-back launches per window, median of WARM_REPS windows per form, per launch.
Form 0 (deconv_direct_f32) is timed twice, as two separate candidates: the difference is the run-to-run spread every other difference is
judged against. The static rule may name a bf16-plane form only where it is not above form 0 by more than form 0's own spread on BOTH
protocols. Bytes are input + output + weights from the shapes; the share is of the 8 TB/s HBM peak. Rows: U-Net decoder ups (k2 s2),
generator ups (k4 s2 p1), one k3 s2 p1; batch 1, and batch 8 where the output stays below 256 MB.
Each step is one process with its own exit status: run it under `timeout`."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

ROWS = [(1024, 512, 28, 2, 0), (512, 256, 56, 2, 0), (256, 128, 112, 2, 0), (128, 64, 224, 2, 0),      # C, K, H, k, pad (stride 2)
        (512, 256, 8, 4, 1), (256, 128, 16, 4, 1), (128, 64, 32, 4, 1), (64, 32, 64, 4, 1),
        (256, 128, 28, 3, 1)]
HBM_PEAK = 8.0e12
REPS, WARM_REPS, WARM_LAUNCHES = 25, 7, 10
NAMES = ["deconv_direct_f32", "deconv_b3_f32_4x16", "deconv_b3_f32_2x16"]


def shapes(out_dir):
    import torch
    from anakin_amd import lib as L
    from anakin_amd import saber as S
    L.require_device()
    torch.cuda.set_stream(torch.cuda.Stream())
    rng = np.random.default_rng(0)
    flush = torch.ones(16 << 20, dtype=torch.float32, device="cuda")      # 64 MB
    sink = torch.zeros(1, dtype=torch.float32, device="cuda")
    rows = []
    for (c, k, h, ks, pad) in ROWS:
        for n in (1, 8):
            oh = (h - 1) * 2 + ks - 2 * pad
            if n * oh * oh * k * 4 >= 256 << 20:
                continue
            w = (rng.standard_normal((c, k, ks, ks)) * 0.05).astype(np.float32)
            b = rng.standard_normal(k).astype(np.float32)
            op = S.SaberDeconv2D().init((n, c, h, h), S.ConvParam(w, b, 1, (pad, pad), (2, 2), (1, 1), True))
            static = op.tile()
            nbytes = 4 * (n * h * h * c + n * oh * oh * k + c * k * ks * ks)
            x = torch.randn((n, h, h, c), device="cuda")
            y = op.new_output()
            cands = [("form0", lambda: op.set_tile(0)), ("form0_again", lambda: op.set_tile(0))] + \
                    [("form%d" % f, (lambda f=f: op.set_tile(f))) for f in op.forms() if f]
            run = {kk: (lambda: op.dispatch(x, y)) for kk, _ in cands}
            names = {}
            if ks == 2:      # the same arithmetic as a 1x1 conv C -> 4K with the existing FP32 kernels (static selection): [n, h, w, 4K]
                w1 = np.ascontiguousarray(w.transpose(2, 3, 1, 0).reshape(4 * k, c, 1, 1))
                conv = S.SaberConv2D(False).init((n, c, h, h), S.ConvParam(w1, np.tile(b, 4), 1, (0, 0), (1, 1), (1, 1), True), L.F32, L.F32,
                                                 in_layout=L.NHWC, out_layout=L.NHWC)
                y1 = conv.new_output()
                cands.append(("conv1x1_4k", lambda: None))
                run["conv1x1_4k"] = lambda: conv.dispatch(x, y1)
                names["conv1x1_4k"] = conv.algo()
            for kk, sel in cands:      # warm-up: code and kernel arguments of every form
                sel()
                if kk not in names:
                    names[kk] = op.algo()
                for _ in range(3):
                    run[kk]()
            torch.cuda.synchronize()
            ev = []
            for _ in range(REPS):
                for kk, sel in cands:
                    sel()
                    sink.add_(flush.sum())
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    run[kk]()
                    e1.record()
                    ev.append((kk, e0, e1))
            torch.cuda.synchronize()
            cold = {kk: [] for kk, _ in cands}
            for kk, e0, e1 in ev:
                cold[kk].append(e0.elapsed_time(e1) * 1000.0)
            ev = []
            for _ in range(WARM_REPS):
                for kk, sel in cands:
                    sel()
                    run[kk]()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(WARM_LAUNCHES):
                        run[kk]()
                    e1.record()
                    ev.append((kk, e0, e1))
            torch.cuda.synchronize()
            warm = {kk: [] for kk, _ in cands}
            for kk, e0, e1 in ev:
                warm[kk].append(e0.elapsed_time(e1) * 1000.0 / WARM_LAUNCHES)
            op.set_tile(static)
            row = dict(c=c, k=k, h=h, ks=ks, pad=pad, batch=n, bytes=nbytes, static_form=static,
                       us={kk: float(np.median(v)) for kk, v in cold.items()}, us_warm={kk: float(np.median(v)) for kk, v in warm.items()}, kernel=names)
            rows.append(row)
            print(json.dumps(row), flush=True)
    os.makedirs(out_dir, exist_ok=True)
    json.dump(rows, open(os.path.join(out_dir, "shapes.json"), "w"), indent=1)


def _row_batches():
    for (c, k, h, ks, pad) in ROWS:
        for n in (1, 8):
            oh = (h - 1) * 2 + ks - 2 * pad
            if n * oh * oh * k * 4 < 256 << 20:
                yield c, k, h, ks, pad, n


def check(out_dir):
    """the shapes of shapes.json, which are the ones create names a bf16-plane form for, compared with a reference (the timing runs compare
    nothing). A batch-8 row is compared on its first and its last image: that covers the batch stride, and the float64 rule stays at two
    images a row."""
    import torch
    from anakin_amd import lib as L
    from anakin_amd import saber as S
    from tests import deconv_util as DU
    L.require_device()
    rng = np.random.default_rng(0)
    lines, bad = ["# scripts/bench_deconv.py check: f32 NHWC, bias and relu, stride 2; every accepted form once against the float64 rule "
                  "(tests/deconv_util.py deconv_ref)",
                  "# criteria: the largest error over the largest value, and every error over |value| + mean |value|, both <= 1e-4; forms 1 and 2 byte for byte",
                  "# a batch-8 row is compared on its first and its last image (the batch stride); a batch-1 row in full"], 0
    for (c, k, h, ks, pad, n) in _row_batches():
        cs = DU.case(n, h, h, c, k, ks, pad=(pad, pad))
        x, w, b = DU.make(cs, rng)
        w *= np.float32(1.0 / (0.3 * np.sqrt(c)))
        op = S.SaberDeconv2D().init((n, c, h, h), S.ConvParam(w, b, 1, (pad, pad), (2, 2), (1, 1), True))
        static, forms = op.tile(), op.forms()
        images = sorted({0, n - 1})
        want = DU.deconv_ref(x[images], w, b, dict(cs, n=len(images)), True)
        xd = torch.from_numpy(np.ascontiguousarray(x.transpose(0, 2, 3, 1))).cuda()
        tag = "%d -> %d @ %d^2 k%d p%d batch %d" % (c, k, h, ks, pad, n)
        got = {}
        for f in forms:
            op.set_tile(f)
            y = op.new_output()
            y.fill_(float("nan"))
            op.dispatch(xd, y)
            torch.cuda.synchronize()
            got[f] = y.cpu().numpy()
            try:
                e_max, e_el = DU.fp32_close(got[f][images].transpose(0, 3, 1, 2), want, tag)
                ok = True
            except AssertionError as e:
                (_, e_max, e_el), ok = e.args[0], False
            bad += not ok
            lines.append("%s: form %d %s%s images %s e_max %.3g e_el %.3g %s" % (tag, f, NAMES[f], " (static)" if f == static else "", images, e_max, e_el,
                                                                                 "ok" if ok else "FAILED"))
            print(lines[-1], flush=True)
        same = got[1].tobytes() == got[2].tobytes() if 1 in got and 2 in got else None
        bad += same is not True or forms != [0, 1, 2]
        lines.append("%s: forms %s; forms 1 and 2 byte for byte over all %d images: %s" % (tag, forms, n, {True: "identical", False: "DIFFERENT", None: "NOT RUN"}[same]))
        print(lines[-1], flush=True)
        op.set_tile(static)
    lines.append("%d row x batch combinations, %d failures" % (len(list(_row_batches())), bad))
    print(lines[-1])
    os.makedirs(out_dir, exist_ok=True)
    open(os.path.join(out_dir, "check.txt"), "w").write("\n".join(lines) + "\n")
    return 1 if bad else 0


def _judge(r):
    """(form 0 cold, cold spread, form 0 warm, warm spread, {b3 form: within form 0's spread on both protocols})"""
    us, uw = r["us"], r["us_warm"]
    spread, wspread = abs(us["form0"] - us["form0_again"]), abs(uw["form0"] - uw["form0_again"])
    m0, w0 = (us["form0"] + us["form0_again"]) / 2, (uw["form0"] + uw["form0_again"]) / 2
    ok = {f: us[f] <= m0 + spread and uw[f] <= w0 + wspread for f in ("form1", "form2") if f in us}
    return m0, spread, w0, wspread, ok


def static_form(r):
    """what saber_hip_deconv2d_create selects for a row NOW (host side, no device needed)"""
    import ctypes as C
    from anakin_amd import lib as L
    lib = L.load()
    d = L.ConvDesc()
    d.n, d.h, d.w, d.c, d.k, d.kh, d.kw = r["batch"], r["h"], r["h"], r["c"], r["k"], r["ks"], r["ks"]
    d.pad_h = d.pad_w = r["pad"]
    d.stride_h = d.stride_w = 2
    d.dil_h = d.dil_w = d.group = 1
    d.in_dtype = d.out_dtype = L.F32
    d.in_layout = d.out_layout = L.NHWC
    d.act = L.ACT_RELU
    h = C.c_void_p()
    L.check(lib.saber_hip_deconv2d_create(C.byref(d), C.byref(h)))
    form = lib.saber_hip_deconv2d_get_tile(h)
    lib.saber_hip_deconv2d_destroy(h)
    return form


def table(out_dir):
    rows = json.load(open(os.path.join(out_dir, "shapes.json")))
    out = ["# Deconv kernels, measured", "",
           "Written by `scripts/bench_deconv.py table` from `shapes.json` (MI355X; f32 NHWC, bias and relu; stride 2; forms alternating in one process).",
           "`cold`: one launch per window after a 64 MB stream through the L2s, median of %d; `warm`: %d back-to-back launches per window, median" % (REPS, WARM_LAUNCHES),
           "of %d, per launch. `form0` is `deconv_direct_f32`, timed twice: `spread` is the difference of the two medians. `form1` / `form2` are" % WARM_REPS,
           "`deconv_b3_f32_4x16` / `_2x16`. `conv1x1` (k2 rows) is the same arithmetic through the existing FP32 1x1 conv C -> 4K with its static",
           "selection: the same bytes, the output not pixel-shuffled. `MB` is input + output + weights; `share` is those bytes over the cold time of the",
           "fastest deconv form against the 8 TB/s HBM peak. `within` lists the bf16-plane forms that are not above form 0 (mean of the two) by more",
           "than form 0's spread on BOTH protocols - the only forms the static rule (`deconv_static_form`, api_deconv.hip) may name; `static` is what",
           "`saber_hip_deconv2d_create` selects, `ok` that it is form 0 or one of those.", "",
           "| C -> K | H | k / pad | batch | MB | cold form0 | again | spread | form1 | form2 | conv1x1 | warm form0 | again | spread | form1 | form2 | conv1x1 | best deconv | share | within | static | ok |",
           "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    bad, rule, losing, conv_wins = 0, [], [], []
    for r in rows:
        us, uw = r["us"], r["us_warm"]
        m0, spread, w0, wspread, ok = _judge(r)
        forms = ["form0"] + sorted(ok)
        best = min(forms, key=lambda f: min(us["form0"], us["form0_again"]) if f == "form0" else us[f])
        tb = (min(us["form0"], us["form0_again"]) if best == "form0" else us[best]) * 1e-6
        within = [f for f in sorted(ok) if ok[f]]
        st = "form%d" % static_form(r)      # (the library as it is now, not as it was when the row was measured)
        st_ok = st == "form0" or st in within
        bad += not st_ok
        tag = "%d -> %d @ %d^2 k%d p%d batch %d" % (r["c"], r["k"], r["h"], r["ks"], r["pad"], r["batch"])
        if within:
            pick = min(within, key=lambda f: us[f])
            rule.append("{%d, %d, %d, %d, %d, %d, %s}, // %s: %.1f us against %.1f (cold), %.1f against %.1f (warm)" % (
                r["batch"], r["h"], r["c"], r["k"], r["ks"], r["pad"], pick[4:], tag, us[pick], m0, uw[pick], w0))
        for f in sorted(ok):
            if not ok[f]:
                losing.append("%s: %s %.1f us cold / %.1f warm against form 0's %.1f +- %.1f / %.1f +- %.1f" % (tag, f, us[f], uw[f], m0, spread, w0, wspread))
        c1 = us.get("conv1x1_4k")
        if c1 is not None and c1 < min(us[f] for f in us if f != "conv1x1_4k") and uw["conv1x1_4k"] < min(uw[f] for f in uw if f != "conv1x1_4k"):
            conv_wins.append("%s: `%s` %.1f us cold / %.1f warm; the fastest deconv form %.1f / %.1f" % (
                tag, r["kernel"]["conv1x1_4k"], c1, uw["conv1x1_4k"], min(us[f] for f in us if f != "conv1x1_4k"), min(uw[f] for f in uw if f != "conv1x1_4k")))
        fmt = lambda d, f: "%.1f" % d[f] if f in d else "-"
        out.append("| %d -> %d | %d | %d / %d | %d | %.1f | %.1f | %.1f | %.1f | %s | %s | %s | %.1f | %.1f | %.1f | %s | %s | %s | %s | %.1f %% | %s | %s | %s |" % (
            r["c"], r["k"], r["h"], r["ks"], r["pad"], r["batch"], r["bytes"] / 1e6, us["form0"], us["form0_again"], spread, fmt(us, "form1"), fmt(us, "form2"),
            fmt(us, "conv1x1_4k"), uw["form0"], uw["form0_again"], wspread, fmt(uw, "form1"), fmt(uw, "form2"), fmt(uw, "conv1x1_4k"), best,
            100 * r["bytes"] / tb / HBM_PEAK, ", ".join(within) or "none", st, "yes" if st_ok else "NO"))
    out += ["", "All times in microseconds.", "", "## Rows the static rule may name (C++ initialisers of `deconv_static_form`'s table: batch, H, C, K, k, pad, form)", ""]
    out += ["```"] + (rule or ["(none)"]) + ["```", "", "## Rows where a bf16-plane form loses to form 0 (never named; they run form 0 unless autotuned)", ""]
    out += ["- " + s for s in losing] or ["None."]
    out += ["", "## k2 rows where the existing 1x1 conv route beats every deconv form on both protocols", ""]
    out += ["- " + s for s in conv_wins] or ["None."]
    out += ["", "The 1x1 route writes [n, h, w, 4K]: a consumer that needs the upsampled [n, 2h, 2w, K] tensor pays one more pass over the output for the",
            "pixel shuffle, which the figures above do not include.", ""]
    open(os.path.join(out_dir, "README.md"), "w").write("\n".join(out))
    print("\n".join(out))
    return 1 if bad else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("step", choices=["shapes", "table", "check"])
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "deconv"))
    a = ap.parse_args()
    sys.exit({"shapes": lambda: shapes(a.out), "table": lambda: table(a.out), "check": lambda: check(a.out)}[a.step]() or 0)
