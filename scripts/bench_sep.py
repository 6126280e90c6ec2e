"""The separable launch (conv_sep.hip: depthwise 3x3 + pointwise 1x1 INT8 in one launch) against the two tuned launches it replaces,
and MobileNet-v1 INT8 with and without saber_hip_net_optimize flag 16384.

  python scripts/bench_sep.py shapes [--out DIR]    the distinct (C, H, stride, K) pairs of MobileNet-v1 x batch 1 / 8 (u8 -> u8 -> u8)
  python scripts/bench_sep.py nets   [--out DIR]    MobileNet-v1 INT8, batch 1 / 8, captured and replayed: without the flag (the selection
                                                    every net had before) and with it, static and autotuned
  python scripts/bench_sep.py table  [--out DIR]    DIR/shapes.json + DIR/nets.json -> DIR/README.md (no GPU needed)

`shapes` puts each pair into a two-op net with the flag, lets saber_hip_net_autotune tune the two ops, and then times every
candidate in ONE process, alternating between them, with device events and the operands cold in L2 (a 64 MB stream through the L2s
between two timed launches, as the autotuner's ColdBench does): the two separate launches TWICE, as two candidates - their difference
is the run's spread - and every form of the one launch. A form wins a shape only where it is below both timings of the separate
launches by more than that spread; sep_static_form (api_sep.hip) names it for those of the winning rows whose margin is at least
MARGIN (10 %), keyed on the exact (C, H, stride, K, batch) of the row.
Each step is one process with its own exit status: run it under `timeout`."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

REPS = 15
MARGIN = 1.10      # sep_static_form's extra condition on a winning row: separate / form >= MARGIN
SEP_FLAG = 16384


def mobilenet_pairs():
    """the distinct (C, H, stride, K) of MobileNet-v1's depthwise + pointwise pairs at 224 x 224, in network order"""
    from anakin_amd import workloads as W
    spec = [l for l in W.mobilenet_v1_spec() if l["kind"] == "conv"]
    hw, out = 224, []
    for a, b in zip(spec, spec[1:] + [None]):
        ho = (hw + 2 * a["pad"] - a["k"]) // a["stride"] + 1
        if a.get("group", 1) > 1:
            assert b is not None and b["src"] == a["name"] and b["k"] == 1
            p = (a["cin"], hw, a["stride"], b["cout"])
            if p not in out:
                out.append(p)
        hw = ho
    return out


def _pair_net(S, L, rng, n, c, h, s, k):
    w1 = (rng.standard_normal((c, 1, 3, 3)) * 0.4).astype(np.float32)
    w2 = (rng.standard_normal((k, c, 1, 1)) / np.sqrt(c)).astype(np.float32)
    b1, b2 = rng.standard_normal(c).astype(np.float32), rng.standard_normal(k).astype(np.float32)
    lay = dict(in_layout=L.NHWC, out_layout=L.NHWC)
    dw = S.SaberConv2D(True).init((n, c, h, h), S.ConvParam(w1, b1, c, (1, 1), (s, s), (1, 1), True), L.U8, L.U8, 0.02, 0.05, **lay)
    ho = dw.out_hw[0]
    pw = S.SaberConv2D(True).init((n, c, ho, ho), S.ConvParam(w2, b2, 1, (0, 0), (1, 1), (1, 1), True), L.U8, L.U8, 0.05, 0.05, **lay)
    net = S.Net()
    net.add_tensor("x", (n, h, h, c), L.U8)
    net.add_tensor("mid", (n, ho, ho, c), L.U8)
    net.add_tensor("y", (n, ho, ho, k), L.U8)
    net.add_conv(dw, "x", "mid")
    net.add_conv(pw, "mid", "y")
    assert net.optimize(SEP_FLAG) == 1
    net.finalize()
    return net


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
    for (c, h, s, k) in mobilenet_pairs():
        for n in (1, 8):
            net = _pair_net(S, L, rng, n, c, h, s, k)
            x = net.tensor("x")
            x.copy_((torch.rand(x.shape, device="cuda") * 200).to(x.dtype))
            net.run()
            net.autotune(iters=7)
            tuned = (net.choices()[0] >> 24) & 15
            base = net.choices()[0] & 0xffffff
            forms = [f for f in range(1, 16) if lib.saber_hip_net_set_choice(net.h, 0, base | (3 << 28) | (f << 24)) == 0]
            cands = [("separate", 0), ("separate_again", 0)] + [("form%d" % f, f) for f in forms]
            names, t = {}, {key: [] for key, _ in cands}
            work = {}
            for key, f in cands:      # warm-up: code and kernel arguments of every candidate
                L.check(lib.saber_hip_net_set_choice(net.h, 0, base | (3 << 28) | (f << 24)))
                names[key] = " + ".join(net.op_name(i)[5:] for i in range(2)) if not f else net.op_name(0)[5:]
                work[key] = net.op_work(0)[0] + net.op_work(1)[0]
                for _ in range(3):
                    net.run()
            torch.cuda.synchronize()
            ev = [(key, torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(REPS) for key, _ in cands]
            i = 0
            for _ in range(REPS):
                for key, f in cands:
                    L.check(lib.saber_hip_net_set_choice(net.h, 0, base | (3 << 28) | (f << 24)))
                    sink.add_(flush.sum())
                    ev[i][1].record()
                    net.run()
                    ev[i][2].record()
                    i += 1
            torch.cuda.synchronize()
            for key, e0, e1 in ev:
                t[key].append(e0.elapsed_time(e1) * 1000.0)
            us = {key: float(np.median(v)) for key, v in t.items()}
            row = dict(c=c, h=h, stride=s, k=k, batch=n, us=us, kernel=names, autotuned_form=tuned, bytes=work["separate"])
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
    model = W.build_model("mobilenet_v1")
    fw = W.framework_model(model, "int8")
    rows = []
    for batch in (1, 8):
        x = W.make_input(batch)
        scales = W.calibrate(model, x)
        built = {}
        for label, sep in (("plain", False), ("separable", True)):
            net = W.build_int8_net(fw, dict(scales), batch, separable=sep)
            net.tensor("data").copy_(torch.from_numpy(x).cuda())
            net.run()
            static = net.choices()
            net.autotune(iters=7)
            built[label] = (net, static, net.choices())
        ms, launches, on = {}, {}, {}
        for rep in range(2):      # every configuration twice, alternating: the second round shows the spread
            for label, (net, static, tuned) in built.items():
                for sel, ch in (("static", static), ("autotuned", tuned)):
                    net.set_choices(ch)
                    key = label + "_" + sel
                    ms.setdefault(key, []).append(_replay_ms(net))
                    launches[key] = net.num_launches()
                    on[key] = [(net.op_name(i)[5:]) for i, c in enumerate(ch) if (c >> 28) & 3 == 3 and (c >> 24) & 15]
        row = dict(model="mobilenet_v1", precision="int8", batch=batch, ms=ms, launches=launches, sites_on=on)
        rows.append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(out_dir, exist_ok=True)
    json.dump(rows, open(os.path.join(out_dir, "nets.json"), "w"), indent=1)


def table(out_dir):
    rows = json.load(open(os.path.join(out_dir, "shapes.json")))
    forms = sorted({key for r in rows for key in r["us"] if key.startswith("form")}, key=lambda s: int(s[4:]))
    out = ["# Separable launch: `conv_sep.hip` against the two tuned launches it replaces", "",
           "Written by `scripts/bench_sep.py table` from `shapes.json` / `nets.json` (MI355X, cold-L2 medians of %d runs per candidate," % REPS,
           "candidates alternating in one process, u8 -> u8 -> u8 with bias and relu on both ops). `separate` is the depthwise launch + the",
           "pointwise launch, both tuned by `saber_hip_net_autotune`, timed twice: `spread` is the difference of the two. A form `wins` a",
           "row only where it is below BOTH separate timings by more than the spread. `static` is what `sep_static_form` (api_sep.hip) does",
           "with the row: it names the best form where the row is won by at least %d %% (`formN`), and answers 0 = two launches where the" % round((MARGIN - 1) * 100),
           "row is won by less (`off: under the margin`) or lost (`off`). The rule keys on the exact (C, H, stride, K, batch) of a row: other",
           "batch sizes and resolutions get two launches unless the net is autotuned.",
           "`-`: the form does not exist for that pair (a K-splitting form needs more than one slice).", "",
           "| C | H | stride | K | batch | separate us | again | spread | " + " | ".join("%s us" % f for f in forms) + " | best form | wins | static | autotuner kept |",
           "|---|---|---|---|---|---|---|---|" + "---|" * len(forms) + "---|---|---|---|"]
    wins = named = 0
    for r in rows:
        us = r["us"]
        sep_lo, spread = min(us["separate"], us["separate_again"]), abs(us["separate"] - us["separate_again"])
        have = [f for f in forms if f in us]
        best = min(have, key=lambda f: us[f])
        win = us[best] < sep_lo - spread
        wins += win
        static = best if win and sep_lo / us[best] >= MARGIN else ("off: under the margin" if win else "off")
        named += static == best
        out.append("| %d | %d | %d | %d | %d | %.2f | %.2f | %.2f | %s | %s | %s | %s | %s |" % (
            r["c"], r["h"], r["stride"], r["k"], r["batch"], us["separate"], us["separate_again"], spread,
            " | ".join("%.2f" % us[f] if f in us else "-" for f in forms), best, "yes (%.2fx)" % (sep_lo / us[best]) if win else "no", static,
            "form%d" % r["autotuned_form"] if r["autotuned_form"] else "separate"))
    k0 = max(rows, key=lambda r: len(r["kernel"]))["kernel"]
    out += ["", "%d of %d rows are won by a form of the one launch; the static rule names a form for %d of them." % (wins, len(rows), named), "",
            "Forms: " + ", ".join("%s = `%s`" % (f, k0[f]) for f in forms if f in k0) + ".", ""]
    np_ = os.path.join(out_dir, "nets.json")
    if os.path.exists(np_):
        out += ["## MobileNet-v1 INT8, captured and replayed", "",
                "`plain` is the net without flag 16384 - the selection every net had before this kernel existed - measured in the same process;",
                "two replay timings per configuration (ms per pass), launches per pass, and the sites that run the one launch.",
                "`separable_static` is what `sep_static_form` selects for this net, `separable_autotuned` what `saber_hip_net_autotune` keeps.",
                "(`shapes` and `nets` are separate steps: the rule was written from the table above, then `nets` was run with it.)", "",
                "| batch | configuration | ms / pass | launches | sites on |", "|---|---|---|---|---|"]
        for r in json.load(open(np_)):
            for key in ("plain_static", "separable_static", "plain_autotuned", "separable_autotuned"):
                out.append("| %d | %s | %s | %d | %d |" % (r["batch"], key, " / ".join("%.4f" % v for v in r["ms"][key]), r["launches"][key],
                                                          len(r["sites_on"][key])))
        out.append("")
    open(os.path.join(out_dir, "README.md"), "w").write("\n".join(out))
    print("\n".join(out))
    return 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("step", choices=["shapes", "nets", "table"])
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "sep"))
    a = ap.parse_args()
    sys.exit({"shapes": lambda: shapes(a.out), "nets": lambda: nets(a.out), "table": lambda: table(a.out)}[a.step]() or 0)
