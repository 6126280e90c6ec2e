"""Grouped 3x3 INT8 kernels (conv_group3x3.hip, selection variant 17) against the direct kernel they replace, and ResNeXt-50 with and
without them.

  python scripts/bench_group.py shapes [--out DIR]   the seven grouped layers of ResNeXt-50 32x4d x batch 1 / 8 (u8 -> u8, relu)
  python scripts/bench_group.py nets   [--out DIR]   ResNeXt-50 INT8, batch 1 / 8, captured and replayed: the static selection against
                                                     the 16 grouped ops forced to form 0
  python scripts/bench_group.py table  [--out DIR]   DIR/shapes.json + DIR/nets.json -> DIR/measured.md (no GPU needed); exit status 1
                                                     when one of the two timing conditions of the write-up does not hold

`shapes` times every selectable form of each op in ONE process, alternating between the forms, after a warm-up, with device events:
  cold  one launch per window with the operands cold in L2 - between two timed launches a 64 MB buffer is streamed through the L2s, as the
        autotuner's ColdBench does (the 256 MB Infinity Cache keeps the operands) - median of REPS windows per form;
  warm  WARM_LAUNCHES back-to-back launches per window, median of WARM_REPS windows per form, per launch.
Form 0 (the direct kernel) is timed twice, as two separate candidates: the difference is the run-to-run spread every other difference
is judged against. `table` judges the static choice on BOTH protocols: not above form 0 by more than form 0's own spread in the cold
figures and in the warm ones. Bytes are input + output + weights computed from the shapes; the share is of the 8 TB/s HBM peak.
Each step is one process with its own exit status: run it under `timeout`."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

SHAPES = [(128, 4, 56, 1), (256, 8, 56, 2), (256, 8, 28, 1), (512, 16, 28, 2), (512, 16, 14, 1), (1024, 32, 14, 2), (1024, 32, 7, 1)]      # C, Cg, H, stride
HBM_PEAK = 8.0e12
REPS, WARM_REPS, WARM_LAUNCHES = 25, 7, 20
V = 17


def _forms(lib, conv):
    v, out = 1, []
    while lib.saber_hip_conv2d_set_tile(conv.h, (V << 16) | v) == 0:
        out.append(v)
        v += 1
    return out


def shapes(out_dir):
    import torch
    from anakin_amd import lib as L
    from anakin_amd import saber as S
    L.require_device()
    lib = L.load()
    torch.cuda.set_stream(torch.cuda.Stream())
    rng = np.random.default_rng(0)
    flush = torch.ones(16 << 20, dtype=torch.float32, device="cuda")      # 64 MB
    sink = torch.zeros(1, dtype=torch.float32, device="cuda")
    rows = []
    for (c, cg, h, s) in SHAPES:
        for n in (1, 8):
            w = (rng.standard_normal((c, cg, 3, 3)) * 0.4).astype(np.float32)
            b = rng.standard_normal(c).astype(np.float32)
            prm = S.ConvParam(w, b, c // cg, (1, 1), (s, s), (1, 1), True)
            conv = S.SaberConv2D(True).init((n, c, h, h), prm, L.U8, L.U8, 0.02, 0.05, in_layout=L.NHWC, out_layout=L.NHWC)
            static = lib.saber_hip_conv2d_get_tile(conv.h) & 0xff
            ho = conv.out_hw[0]
            nbytes = n * h * h * c + n * ho * ho * c + c * cg * 9
            x = (torch.rand((n, h, h, c), device="cuda") * 200).to(torch.uint8)
            y = conv.new_output()
            cands = [("form0", 0), ("form0_again", 0)] + [("form%d" % v, v) for v in _forms(lib, conv)]
            names = {}
            for k, v in cands:      # warm-up: code and kernel arguments of every form
                conv.set_tile((V << 16) | v)
                names[k] = conv.algo()
                for _ in range(3):
                    conv.dispatch(x, y)
            torch.cuda.synchronize()
            ev = []
            for _ in range(REPS):
                for k, v in cands:
                    conv.set_tile((V << 16) | v)
                    sink.add_(flush.sum())
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    conv.dispatch(x, y)
                    e1.record()
                    ev.append((k, e0, e1))
            torch.cuda.synchronize()
            cold = {k: [] for k, _ in cands}
            for k, e0, e1 in ev:
                cold[k].append(e0.elapsed_time(e1) * 1000.0)
            ev = []
            for _ in range(WARM_REPS):
                for k, v in cands:
                    conv.set_tile((V << 16) | v)
                    conv.dispatch(x, y)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(WARM_LAUNCHES):
                        conv.dispatch(x, y)
                    e1.record()
                    ev.append((k, e0, e1))
            torch.cuda.synchronize()
            warm = {k: [] for k, _ in cands}
            for k, e0, e1 in ev:
                warm[k].append(e0.elapsed_time(e1) * 1000.0 / WARM_LAUNCHES)
            us = {k: float(np.median(v)) for k, v in cold.items()}
            row = dict(c=c, cg=cg, h=h, stride=s, batch=n, bytes=nbytes, static_form=static, us=us,
                       us_warm={k: float(np.median(v)) for k, v in warm.items()}, kernel=names)
            rows.append(row)
            print(json.dumps(row), flush=True)
    os.makedirs(out_dir, exist_ok=True)
    json.dump(rows, open(os.path.join(out_dir, "shapes.json"), "w"), indent=1)


def _replay_ms(net, iters=50):
    import torch
    net.capture()
    for _ in range(5):
        net.replay()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        net.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def nets(out_dir):
    import torch
    from anakin_amd import lib as L
    from anakin_amd import workloads as W
    L.require_device()
    torch.cuda.set_stream(torch.cuda.Stream())
    model = W.build_model("resnext50_32x4d")
    rows = []
    for batch in (1, 8):
        x = W.make_input(batch)
        net = W.build_int8_net(W.framework_model(model, "int8"), W.calibrate(model, x), batch)
        net.tensor("data").copy_(torch.from_numpy(x).cuda())
        net.run()
        static = net.choices()
        gi = [i for i, c in enumerate(static) if (c >> 16) & 0xff == V]
        assert len(gi) == 16, gi
        direct = [(V << 16) if i in gi else c for i, c in enumerate(static)]
        ms = {}
        for rep in range(3):      # static, direct, static, direct, ...: the repeats show the spread
            for label, ch in (("static", static), ("group_ops_on_form0", direct)):
                net.set_choices(ch)
                ms.setdefault(label, []).append(_replay_ms(net))
        net.set_choices(static)
        row = dict(model="resnext50_32x4d", precision="int8", batch=batch, launches=net.num_launches(), ops=net.num_ops(), ms=ms,
                   group_kernels=sorted({net.op_name(i) for i in gi}))
        rows.append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(out_dir, exist_ok=True)
    json.dump(rows, open(os.path.join(out_dir, "nets.json"), "w"), indent=1)


def table(out_dir):
    rows = json.load(open(os.path.join(out_dir, "shapes.json")))
    forms = sorted(k for k in rows[0]["us"] if k not in ("form0", "form0_again"))
    out = ["Written by `scripts/bench_group.py table` from `shapes.json` / `nets.json` (MI355X; u8 -> u8 with relu and bias; forms alternating",
           "in one process). `cold`: one launch per window after a 64 MB stream through the L2s, median of %d; `warm`: %d back-to-back" % (REPS, WARM_LAUNCHES),
           "launches per window, median of %d, per launch. `form0` is `conv_direct_kernel`, timed twice: `spread` is the difference of the two" % WARM_REPS,
           "cold medians. `GB/s` and `share` are input + output + weight bytes over the cold time of the fastest form, against the 8 TB/s HBM",
           "peak. `static` is what `saber_hip_conv2d_create` selects; `ok` says that its time is not above form 0's (mean of the two) by more than",
           "form 0's spread - in the cold figures AND in the warm ones (`warm spread` is the difference of form 0's two warm medians).", "",
           "| C | Cg | H | stride | batch | KB | form0 us | again | spread | " + " | ".join("%s us" % k for k in forms) + " | warm form0 | warm again | warm spread | " +
           " | ".join("warm %s" % k for k in forms) + " | best | GB/s | share | static | ok |",
           "|---|---|---|---|---|---|---|---|---|" + "---|" * (2 * len(forms) + 3) + "---|---|---|---|---|"]
    bad = 0
    for r in rows:
        us, uw = r["us"], r["us_warm"]
        f0, spread = min(us["form0"], us["form0_again"]), abs(us["form0"] - us["form0_again"])
        best = min(["form0"] + forms, key=lambda k: f0 if k == "form0" else us[k])
        st = "form%d" % r["static_form"]
        st_us = f0 if st == "form0" else us[st]
        wspread = abs(uw["form0"] - uw["form0_again"])
        st_warm = min(uw["form0"], uw["form0_again"]) if st == "form0" else uw[st]
        ok = st_us <= (us["form0"] + us["form0_again"]) / 2 + spread and st_warm <= (uw["form0"] + uw["form0_again"]) / 2 + wspread
        bad += (not ok) and r["batch"] == 8
        tb = min(f0, *[us[k] for k in forms]) * 1e-6
        out.append("| %d | %d | %d | %d | %d | %.0f | %.2f | %.2f | %.2f | %s | %.2f | %.2f | %.2f | %s | %s | %.0f | %.1f %% | %s | %s |" % (
            r["c"], r["cg"], r["h"], r["stride"], r["batch"], r["bytes"] / 1024, us["form0"], us["form0_again"], spread,
            " | ".join("%.2f" % us[k] for k in forms), uw["form0"], uw["form0_again"], wspread, " | ".join("%.2f" % uw[k] for k in forms), best,
            r["bytes"] / tb / 1e9, 100 * r["bytes"] / tb / HBM_PEAK, st, "yes" if ok else "NO"))
    names = rows[0]["kernel"]
    out += ["", "Kernels: " + ", ".join("%s = `%s`" % (k, names[k]) for k in sorted(names) if k != "form0_again") + ".", ""]
    np_ = os.path.join(out_dir, "nets.json")
    if os.path.exists(np_):
        out += ["ResNeXt-50 32x4d INT8, default fusions, captured and replayed (50 replays per figure, the two selections alternating):", "",
                "| batch | launches | static ms / pass | grouped ops on form 0, ms / pass | spread | gain | ok |", "|---|---|---|---|---|---|---|"]
        for r in json.load(open(np_)):
            a, b = r["ms"]["static"], r["ms"]["group_ops_on_form0"]
            spread = max(max(a) - min(a), max(b) - min(b))
            gain = float(np.median(b) - np.median(a))
            ok = gain > spread
            bad += (not ok) and r["batch"] == 8
            out.append("| %d | %d | %s | %s | %.3f | %.3f ms (x %.2f) | %s |" % (r["batch"], r["launches"], " / ".join("%.3f" % v for v in a),
                                                                              " / ".join("%.3f" % v for v in b), spread, gain,
                                                                              np.median(b) / np.median(a), "yes" if ok else "NO"))
        out.append("")
    open(os.path.join(out_dir, "measured.md"), "w").write("\n".join(out))
    print("\n".join(out))
    return 1 if bad else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("step", choices=["shapes", "nets", "table"])
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "group3x3"))
    a = ap.parse_args()
    sys.exit({"shapes": lambda: shapes(a.out), "nets": lambda: nets(a.out), "table": lambda: table(a.out)}[a.step]() or 0)
