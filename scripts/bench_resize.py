"""The resize kernels (anakin_amd/csrc/resize.hip) against each other, and the fused resize + sum launch against resize followed by
saber_hip_eltwise_sum_f32 as two launches.

  python scripts/bench_resize.py shapes [--out DIR]   every row x batch, every form the op accepts, plain and fused -> DIR/shapes.json
  python scripts/bench_resize.py table  [--out DIR]   DIR/shapes.json -> DIR/README.md (no GPU needed); exit status 1 when the static rules
                                                      (resize_static_form, resize_sum_static_on: api_resize.hip) do not hold on the rows
  python scripts/bench_resize.py check  [--out DIR]   every row x batch once per accepted form, plain and fused, nothing timed: each output
                                                      `==` tests/resize_util.resize_ref (computed on the CPU) -> DIR/check.txt; exit status 1
                                                      when a line fails

The protocol is scripts/bench_deconv.py's: ONE process, the candidates alternating, after a warm-up, with device events:
  cold  one launch (or pair of launches) per window with the operands cold in L2 - between two timed windows a 64 MB buffer is streamed
        through the L2s, as the autotuner's ColdBench does - median of REPS windows per candidate;
  warm  WARM_LAUNCHES back-to-back launches per window, median of WARM_REPS windows per candidate, per launch.
Form 0 (resize_direct_f32) is timed twice, as two separate candidates: the difference is the run-to-run spread. Bytes are input + output
(+ output again for the fused sum's second operand, + 3 x output for the eltwise of the two-launch route); the share is of the 8 TB/s HBM
peak. Rows: FPN top-down, the YOLOv3 neck, segmentation heads, a U-Net bilinear x2; batch 1 and 8.
Each step is one process with its own exit status: run it under `timeout`."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

# (what, C, H = W in, H = W out, mode)
ROWS = [("FPN top-down", 256, 7, 14, 3), ("FPN top-down", 256, 14, 28, 3), ("FPN top-down", 256, 28, 56, 3),
        ("YOLOv3 neck", 256, 13, 26, 3), ("YOLOv3 neck", 128, 26, 52, 3),
        ("seg head x8", 32, 28, 224, 0), ("seg head x8", 32, 28, 224, 1), ("seg head x4", 256, 14, 56, 0), ("seg head x4", 256, 14, 56, 1),
        ("U-Net x2", 64, 112, 224, 1)]
BATCHES = (1, 8)
HBM_PEAK = 8.0e12
REPS, WARM_REPS, WARM_LAUNCHES = 25, 7, 10
NAMES = ["resize_direct_f32", "resize_rows_f32", "resize_x2_f32"]
MARGIN = 0.9      # a form is named only where it is ahead of form 0 by at least a tenth (the separable, block and Fire rules' margin)


def _op(c, h, oh, mode, n):
    from anakin_amd import saber as S
    return S.SaberResize((n, c, h, h), mode, out_h=oh, out_w=oh)


def shapes(out_dir):
    import torch
    from anakin_amd import lib as L
    from anakin_amd import saber as S
    L.require_device()
    torch.cuda.set_stream(torch.cuda.Stream())
    flush = torch.ones(16 << 20, dtype=torch.float32, device="cuda")      # 64 MB
    sink = torch.zeros(1, dtype=torch.float32, device="cuda")
    rows = []
    for (what, c, h, oh, mode) in ROWS:
        for n in BATCHES:
            op = _op(c, h, oh, mode, n)
            static, forms = op.tile(), op.forms()
            x = torch.randn((n, h, h, c), device="cuda")
            b = torch.randn((n, oh, oh, c), device="cuda")
            y, r = op.new_output(), op.new_output()
            cands = [("form0", 0, "plain"), ("form0_again", 0, "plain")] + [("form%d" % f, f, "plain") for f in forms if f]
            cands += [("sum_form%d" % f, f, "sum") for f in forms] + [("two_form%d" % f, f, "two") for f in forms]

            def launch(kind):
                if kind == "plain":
                    op.run(x, y)
                elif kind == "sum":
                    op.run_sum(x, b, y, 1.0, 1.0, False)
                else:
                    op.run(x, r)
                    S.eltwise_sum(r, b, (1.0, 1.0), False, out=y)
            for kk, f, kind in cands:      # warm-up: code and kernel arguments of every candidate
                op.set_tile(f)
                for _ in range(3):
                    launch(kind)
            torch.cuda.synchronize()
            ev = []
            for _ in range(REPS):
                for kk, f, kind in cands:
                    op.set_tile(f)
                    sink.add_(flush.sum())
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    launch(kind)
                    e1.record()
                    ev.append((kk, e0, e1))
            torch.cuda.synchronize()
            cold = {kk: [] for kk, _, _ in cands}
            for kk, e0, e1 in ev:
                cold[kk].append(e0.elapsed_time(e1) * 1000.0)
            ev = []
            for _ in range(WARM_REPS):
                for kk, f, kind in cands:
                    op.set_tile(f)
                    launch(kind)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(WARM_LAUNCHES):
                        launch(kind)
                    e1.record()
                    ev.append((kk, e0, e1))
            torch.cuda.synchronize()
            warm = {kk: [] for kk, _, _ in cands}
            for kk, e0, e1 in ev:
                warm[kk].append(e0.elapsed_time(e1) * 1000.0 / WARM_LAUNCHES)
            op.set_tile(static)
            row = dict(what=what, c=c, h=h, oh=oh, mode=mode, batch=n, bytes=4 * n * c * (h * h + oh * oh), out_bytes=4 * n * c * oh * oh, static_form=static,
                       us={kk: float(np.median(v)) for kk, v in cold.items()}, us_warm={kk: float(np.median(v)) for kk, v in warm.items()})
            rows.append(row)
            print(json.dumps(row), flush=True)
    os.makedirs(out_dir, exist_ok=True)
    json.dump(rows, open(os.path.join(out_dir, "shapes.json"), "w"), indent=1)


def check(out_dir):
    """the shapes of shapes.json compared with resize_ref (the timing runs compare nothing): every form, plain and fused, `==`"""
    import torch
    from anakin_amd import lib as L
    from tests import resize_util as RU
    L.require_device()
    rng = np.random.default_rng(0)
    lines, bad = ["# scripts/bench_resize.py check: f32 NHWC; every accepted form once, plain and with the fused sum (c0 = 0.5, c1 = -1.25, relu), "
                  "against tests/resize_util.py resize_ref / sum_ref", "# criterion: every output bit equal"], 0
    for (what, c, h, oh, mode) in ROWS:
        for n in BATCHES:
            cs = RU.case(n, c, h, h, mode, oh, oh)
            x = RU.make(cs, rng)
            want = RU.resize_ref(x, cs)
            b = rng.standard_normal(want.shape).astype(np.float32)
            want_sum = RU.sum_ref(want, b, 0.5, -1.25, True)
            op = _op(c, h, oh, mode, n)
            static = op.tile()
            xd = torch.from_numpy(np.ascontiguousarray(x.transpose(0, 2, 3, 1))).cuda()
            bd = torch.from_numpy(np.ascontiguousarray(b.transpose(0, 2, 3, 1))).cuda()
            tag = "%s %d @ %d^2 -> %d^2 mode %d batch %d" % (what, c, h, oh, mode, n)
            for f in op.forms():
                op.set_tile(f)
                y = op.new_output()
                y.fill_(float("nan"))
                op.run(xd, y)
                torch.cuda.synchronize()
                ok = y.cpu().numpy().transpose(0, 3, 1, 2).tobytes() == want.tobytes()
                y.fill_(float("nan"))
                op.run_sum(xd, bd, y, 0.5, -1.25, True)
                torch.cuda.synchronize()
                ok_sum = y.cpu().numpy().transpose(0, 3, 1, 2).tobytes() == want_sum.tobytes()
                bad += (not ok) + (not ok_sum)
                lines.append("%s: form %d %s%s plain %s, fused sum %s" % (tag, f, NAMES[f], " (static)" if f == static else "", "identical" if ok else "DIFFERENT",
                                                                         "identical" if ok_sum else "DIFFERENT"))
                print(lines[-1], flush=True)
            bad += op.forms()[:2] != [0, 1]
            op.set_tile(static)
    lines.append("%d row x batch combinations, %d failures" % (len(ROWS) * len(BATCHES), bad))
    print(lines[-1])
    os.makedirs(out_dir, exist_ok=True)
    open(os.path.join(out_dir, "check.txt"), "w").write("\n".join(lines) + "\n")
    return 1 if bad else 0


def static_choice(r):
    """what saber_hip_resize_create selects for a row NOW (host side, no device needed)"""
    import ctypes as C
    from anakin_amd import lib as L
    lib = L.load()
    d = L.ResizeDesc()
    d.n, d.c, d.h, d.w, d.mode, d.out_h, d.out_w = r["batch"], r["c"], r["h"], r["h"], r["mode"], r["oh"], r["oh"]
    d.in_layout = d.out_layout = L.NHWC
    d.dtype = L.F32
    h = C.c_void_p()
    L.check(lib.saber_hip_resize_create(C.byref(d), C.byref(h)))
    form = lib.saber_hip_resize_get_tile(h)
    lib.saber_hip_resize_destroy(h)
    return form


def _ahead(r, f, g):
    """candidate f is ahead of candidate g by at least a tenth on both protocols (form 0: the mean of its two medians)"""
    def t(d, k):
        return (d["form0"] + d["form0_again"]) / 2 if k == "form0" else d[k]
    return t(r["us"], f) <= MARGIN * t(r["us"], g) and t(r["us_warm"], f) <= MARGIN * t(r["us_warm"], g)


def allowed_form(r):
    """the form the measured row allows the static rule to name: 2 where it is ahead of form 1 (and form 1 of form 0), 1 where that is ahead of form 0"""
    if not _ahead(r, "form1", "form0"):
        return 0
    return 2 if "form2" in r["us"] and _ahead(r, "form2", "form1") else 1


def table(out_dir):
    rows = json.load(open(os.path.join(out_dir, "shapes.json")))
    fmt = lambda d, f: "%.1f" % d[f] if f in d else "-"
    out = ["# Resize kernels, measured", "",
           "Written by `scripts/bench_resize.py table` from `shapes.json` (MI355X; f32 NHWC; the candidates alternating in one process).",
           "`cold`: one launch per window after a 64 MB stream through the L2s, median of %d; `warm`: %d back-to-back launches per window, median" % (REPS, WARM_LAUNCHES),
           "of %d, per launch. `form0` is `resize_direct_f32`, timed twice: `spread` is the difference of the two medians; `form1` is `resize_rows_f32`," % WARM_REPS,
           "`form2` is `resize_x2_f32` (integer x2 in modes 1 and 3 only). `MB` is input + output; `share` is those bytes over the cold time of the",
           "fastest form against the 8 TB/s HBM peak; `elems` is the output's element count. `allowed` is the form the row lets the static rule name:",
           "form 1 where it is ahead of form 0 (the mean of its two medians) by at least a tenth on BOTH protocols, form 2 where it is in turn ahead of",
           "form 1 by as much; `static` is what `saber_hip_resize_create` selects (`resize_static_form`, api_resize.hip).", "",
           "| row | C | in -> out | mode | batch | elems | MB | cold form0 | again | spread | form1 | form2 | warm form0 | again | spread | form1 | form2 | share | allowed | static |",
           "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    bad = 0
    for r in rows:
        us, uw = r["us"], r["us_warm"]
        st, al = static_choice(r), allowed_form(r)
        bad += st != al
        tb = min(v for k, v in us.items() if k.startswith("form")) * 1e-6
        out.append("| %s | %d | %d^2 -> %d^2 | %d | %d | %d | %.2f | %.1f | %.1f | %.1f | %.1f | %s | %.1f | %.1f | %.1f | %.1f | %s | %.1f %% | form%d | form%d%s |" % (
            r["what"], r["c"], r["h"], r["oh"], r["mode"], r["batch"], r["out_bytes"] // 4, r["bytes"] / 1e6, us["form0"], us["form0_again"], abs(us["form0"] - us["form0_again"]),
            us["form1"], fmt(us, "form2"), uw["form0"], uw["form0_again"], abs(uw["form0"] - uw["form0_again"]), uw["form1"], fmt(uw, "form2"), 100 * r["bytes"] / tb / HBM_PEAK,
            al, st, "" if st == al else " (NOT the allowed form)"))
    out += ["", "All times in microseconds.", "", "## The fused sum against resize + `eltwise_sum_f32` as two launches", "",
            "`one` is `saber_hip_resize_run_sum`, `two` is `saber_hip_resize_run` followed by `saber_hip_eltwise_sum_f32`, both with the form named in the column;",
            "the one launch moves in + 2 x out floats, the two launches in + 4 x out. `wins`: the one launch is faster on both protocols with EVERY form.", "",
            "| row | C | in -> out | mode | batch | cold one form0 | two form0 | one form1 | two form1 | one form2 | two form2 | warm one form0 | two form0 | one form1 | two form1 | one form2 | two form2 | wins |",
            "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    lost = []
    for r in rows:
        us, uw = r["us"], r["us_warm"]
        forms = [k[4:] for k in us if k.startswith("sum_")]
        wins = all(us["sum_" + f] < us["two_" + f] and uw["sum_" + f] < uw["two_" + f] for f in forms)
        if not wins:
            lost.append("%s %d @ %d^2 -> %d^2 mode %d batch %d" % (r["what"], r["c"], r["h"], r["oh"], r["mode"], r["batch"]))
        out.append("| %s | %d | %d^2 -> %d^2 | %d | %d | %s | %s | %s | %s | %s | %s | %s | %s | %s | %s | %s | %s | %s |" % (
            (r["what"], r["c"], r["h"], r["oh"], r["mode"], r["batch"]) + tuple(fmt(d, k + f) for d in (us, uw) for f in ("form0", "form1", "form2") for k in ("sum_", "two_")) +
            ("yes" if wins else "NO",)))
    n1, n2 = [r for r in rows if allowed_form(r) >= 1], [r for r in rows if allowed_form(r) == 2]
    e = lambda r: r["out_bytes"] // 4
    x2 = [r for r in rows if "form2" in r["us"]]
    out += ["", "## What the static rules follow from", "",
            "- Form 1 is ahead of form 0 by the margin on %d of %d combinations: every one with %d output elements or more and none with %d or fewer." % (
                len(n1), len(rows), min(e(r) for r in n1), max(e(r) for r in rows if allowed_form(r) == 0)),
            "- Form 2 is ahead of form 1 by the margin on %d of the %d x2 combinations: every one with %d output elements or more and none with %d or fewer." % (
                len(n2), len(x2), min(e(r) for r in n2), max(e(r) for r in x2 if allowed_form(r) < 2)) if n2 else
            "- Form 2 is ahead of form 1 by the margin on no x2 combination.",
            "- `resize_static_form` puts one threshold between each pair of figures (1 000 000 and 3 000 000 output elements); every measured combination agrees with them:",
            "  %s." % ("the `static` column equals the `allowed` column on all %d rows" % len(rows) if not bad else "NO - %d rows differ" % bad),
            "- The resize + sum site (flag 131072, `resize_sum_static_on`): the one launch %s." % (
                "wins every measured combination on both protocols with every form, so the site is on by default" if not lost else "does NOT win on: " + "; ".join(lost)), ""]
    open(os.path.join(out_dir, "README.md"), "w").write("\n".join(out))
    print("\n".join(out))
    return 1 if bad or lost else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("step", choices=["shapes", "table", "check"])
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "resize"))
    a = ap.parse_args()
    sys.exit({"shapes": lambda: shapes(a.out), "table": lambda: table(a.out), "check": lambda: check(a.out)}[a.step]() or 0)
