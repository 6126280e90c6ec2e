"""The inverted-residual block launch (conv_ir.hip: 1x1 expand + depthwise 3x3 + 1x1 project [+ eltwise] INT8 in one launch) against the
tuned launches it replaces, and MobileNet-v2 INT8 with and without saber_hip_net_optimize flag 32768.

  python scripts/bench_ir.py blocks [--out DIR]    the 16 expanded blocks of MobileNet-v2 at 224 x 224 x batch 1 / 8
  python scripts/bench_ir.py nets   [--out DIR]    MobileNet-v2 INT8, batch 1 / 8, captured and replayed: without the flag (the selection
                                                   every net had before) and with it, static and autotuned; five alternating runs each
  python scripts/bench_ir.py table  [--out DIR]    DIR/blocks.json + DIR/nets.json -> DIR/README.md (no GPU needed)

`blocks` puts each block into a net of its own - expand, depthwise, project and, where the block has one, the eltwise sum with its
input, which flag 1 fuses into the project conv exactly as the whole network's default path does - adds flag 32768, lets
saber_hip_net_autotune tune the three ops, and then times every candidate in ONE process, alternating between them, with device events
and the operands cold in L2 (a 64 MB stream through the L2s between two timed launches, as the autotuner's ColdBench does): the
separate launches TWICE, as two candidates - their difference is the run's spread - and every form of the one launch. A form wins a
block only where it is below both timings of the separate launches by more than that spread; ir_static_form (api_ir.hip) may name it for
those of the winning rows whose margin is at least MARGIN (10 %), keyed on the exact shape and batch of the row.
Each step is one process with its own exit status: run it under `timeout`."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

REPS = 15
MARGIN = 1.10      # ir_static_form's condition on a winning row: separate / form >= MARGIN
IR_FLAG = 32768
IR_BIT = -(1 << 31)      # bit 31 of the (signed) choice word without bit 30: a block decision


def mobilenet_blocks():
    """(name, Cin, Ce, Cout, H, stride, residual) of MobileNet-v2's 16 expanded blocks at 224 x 224, in network order"""
    from anakin_amd import workloads as W
    spec = W.mobilenet_v2_spec()
    by = {l["name"]: l for l in spec}
    size, out = {"data": 224}, []
    for l in spec:
        if l["kind"] == "conv":
            size[l["name"]] = (size[l["src"]] + 2 * l["pad"] - l["k"]) // l["stride"] + 1
        elif l["kind"] == "eltwise":
            size[l["name"]] = size[l["a"]]
        if l["kind"] == "conv" and l["name"].endswith("_expand"):
            tag = l["name"][:-len("_expand")]
            out.append((tag, l["cin"], l["cout"], by[tag + "_linear"]["cout"], size[l["src"]], by[tag + "_dwise"]["stride"], "eltwise" in by[tag + "_linear"]))
    assert len(out) == 16
    return out


def _block_net(S, L, rng, n, cin, ce, cout, h, s, res):
    lay = dict(in_layout=L.NHWC, out_layout=L.NHWC)
    w1 = (rng.standard_normal((ce, cin, 1, 1)) / np.sqrt(cin)).astype(np.float32)
    w2 = (rng.standard_normal((ce, 1, 3, 3)) * 0.4).astype(np.float32)
    w3 = (rng.standard_normal((cout, ce, 1, 1)) / np.sqrt(ce)).astype(np.float32)
    b1, b2, b3 = (rng.standard_normal(k).astype(np.float32) for k in (ce, ce, cout))
    ex = S.SaberConv2D(True).init((n, cin, h, h), S.ConvParam(w1, b1, 1, (0, 0), (1, 1), (1, 1), True), L.S8, L.U8, 0.02, 0.05, **lay)
    dw = S.SaberConv2D(True).init((n, ce, h, h), S.ConvParam(w2, b2, ce, (1, 1), (s, s), (1, 1), True), L.U8, L.U8, 0.05, 0.05, **lay)
    ho = dw.out_hw[0]
    pr = S.SaberConv2D(True).init((n, ce, ho, ho), S.ConvParam(w3, b3, 1, (0, 0), (1, 1), (1, 1), False), L.U8, L.S8, 0.05, 0.05, **lay)
    net = S.Net()
    net.add_tensor("x", (n, h, h, cin), L.S8)
    net.add_tensor("e", (n, h, h, ce), L.U8)
    net.add_tensor("d", (n, ho, ho, ce), L.U8)
    net.add_tensor("p", (n, ho, ho, cout), L.S8)
    net.add_conv(ex, "x", "e")
    net.add_conv(dw, "e", "d")
    net.add_conv(pr, "d", "p")
    if res:
        net.add_tensor("y", (n, ho, ho, cout), L.S8)
        net.add_eltwise_i8(n * ho * ho * cout, 0.05, 0.02, 1.0 / 0.06, 1.0 / 0.06, False, "p", "x", "y")
        assert net.optimize(1) == 1
    assert net.optimize(IR_FLAG) == 1
    net.finalize()
    assert net.num_ops() == 3
    return net


def blocks(out_dir):
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
    for (tag, cin, ce, cout, h, s, res) in mobilenet_blocks():
        for n in (1, 8):
            net = _block_net(S, L, rng, n, cin, ce, cout, h, s, res)
            x = net.tensor("x")
            x.copy_((torch.rand(x.shape, device="cuda") * 200 - 100).to(x.dtype))
            net.run()
            net.autotune(iters=7)
            tuned = (net.choices()[0] >> 24) & 15
            base = net.choices()[0] & 0xffffff
            word = lambda f: IR_BIT | (f << 24) | base      # noqa: E731
            forms = [f for f in range(1, 8) if lib.saber_hip_net_set_choice(net.h, 0, word(f)) == 0]
            cands = [("separate", 0), ("separate_again", 0)] + [("form%d" % f, f) for f in forms]
            names, t = {}, {key: [] for key, _ in cands}
            for key, f in cands:      # warm-up: code and kernel arguments of every candidate
                L.check(lib.saber_hip_net_set_choice(net.h, 0, word(f)))
                names[key] = " + ".join(net.op_name(i)[5:] for i in range(3)) if not f else net.op_name(0)[5:]
                for _ in range(3):
                    net.run()
            torch.cuda.synchronize()
            ev = [(key, torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(REPS) for key, _ in cands]
            i = 0
            for _ in range(REPS):
                for key, f in cands:
                    L.check(lib.saber_hip_net_set_choice(net.h, 0, word(f)))
                    sink.add_(flush.sum())
                    ev[i][1].record()
                    net.run()
                    ev[i][2].record()
                    i += 1
            torch.cuda.synchronize()
            for key, e0, e1 in ev:
                t[key].append(e0.elapsed_time(e1) * 1000.0)
            us = {key: float(np.median(v)) for key, v in t.items()}
            iqr = {key: float(np.percentile(v, 75) - np.percentile(v, 25)) for key, v in t.items()}
            row = dict(block=tag, cin=cin, ce=ce, cout=cout, h=h, stride=s, residual=bool(res), batch=n, us=us, iqr=iqr, kernel=names, autotuned_form=tuned)
            rows.append(row)
            print(json.dumps(row), flush=True)
    os.makedirs(out_dir, exist_ok=True)
    json.dump(rows, open(os.path.join(out_dir, "blocks.json"), "w"), indent=1)


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
    model = W.build_model("mobilenet_v2")
    fw = W.framework_model(model, "int8")
    rows = []
    for batch in (1, 8):
        x = W.make_input(batch)
        scales = W.calibrate(model, x)
        built = {}
        for label, inv in (("plain", False), ("inverted", True)):
            net = W.build_int8_net(fw, dict(scales), batch, inverted=inv)
            net.tensor("data").copy_(torch.from_numpy(x).cuda())
            net.run()
            static = net.choices()
            net.autotune(iters=7)
            built[label] = (net, static, net.choices())
        ms, launches, on = {}, {}, {}
        for rep in range(5):      # every configuration five times, alternating: the spread between the rounds is the noise
            for label, (net, static, tuned) in built.items():
                for sel, ch in (("static", static), ("autotuned", tuned)):
                    net.set_choices(ch)
                    key = label + "_" + sel
                    ms.setdefault(key, []).append(_replay_ms(net))
                    launches[key] = net.num_launches()
                    on[key] = [(net.op_name(i)[5:]) for i, c in enumerate(ch) if (c >> 30) & 3 == 2 and (c >> 24) & 15]
        f32 = W.build_fp32_net(model, batch)      # context only: the reference's benchmark table has FP32 figures for this model
        f32.tensor("data").copy_(torch.from_numpy(x).cuda())
        f32.run()
        row = dict(model="mobilenet_v2", precision="int8", batch=batch, ms=ms, launches=launches, sites_on=on,
                   fp32_ms=[_replay_ms(f32) for _ in range(3)], fp32_launches=f32.num_launches())
        rows.append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(out_dir, exist_ok=True)
    json.dump(rows, open(os.path.join(out_dir, "nets.json"), "w"), indent=1)


def table(out_dir):
    rows = json.load(open(os.path.join(out_dir, "blocks.json")))
    forms = sorted({key for r in rows for key in r["us"] if key.startswith("form")}, key=lambda s: int(s[4:]))
    out = ["# Inverted-residual block launch: `conv_ir.hip` against the tuned launches it replaces", "",
           "Written by `scripts/bench_ir.py table` from `blocks.json` / `nets.json` (MI355X, cold-L2 medians of %d runs per candidate," % REPS,
           "candidates alternating in one process; s8 -> u8 -> u8 -> s8 with bias on every op, the eltwise sum with the block's input fused into",
           "the project conv by flag 1 where the block has one). `separate` is the expand launch + the depthwise launch + the project launch, all",
           "tuned by `saber_hip_net_autotune` - what the parent commit runs for these ops - timed twice: `spread` is the difference of the",
           "two medians, `iqr` the larger interquartile range of the two. A form `wins` a row only where it is below BOTH separate timings by",
           "more than the spread. `static` is what `ir_static_form` (api_ir.hip) may do with the row: name the best form where the row is won by",
           "at least %d %% (`formN`), and answer 0 = three launches where the row is won by less (`off: under the margin`) or lost (`off`)." % round((MARGIN - 1) * 100),
           "`-`: the form does not exist for that block (form3 needs an output image of at most 16 columns; LDS above 80 KB per workgroup).", "",
           "| block | Cin | Ce | Cout | H | stride | res | batch | separate us | again | spread | iqr | " + " | ".join("%s us" % f for f in forms) +
           " | best form | wins | static | autotuner kept |",
           "|---|---|---|---|---|---|---|---|---|---|---|---|" + "---|" * len(forms) + "---|---|---|---|"]
    wins = named = 0
    rule = []
    for r in rows:
        us = r["us"]
        sep_lo, spread = min(us["separate"], us["separate_again"]), abs(us["separate"] - us["separate_again"])
        have = [f for f in forms if f in us]
        best = min(have, key=lambda f: us[f])
        win = us[best] < sep_lo - spread
        wins += win
        static = best if win and sep_lo / us[best] >= MARGIN else ("off: under the margin" if win else "off")
        if static == best:
            named += 1
            rule.append("    {%d, %d, %d, %d, %d, %d, %s},      // %s: %.2f against %.2f / %.2f (%.2fx)" % (
                r["cin"], r["ce"], r["cout"], r["h"], r["stride"], r["batch"], best[4:], r["block"], us[best], us["separate"], us["separate_again"], sep_lo / us[best]))
        out.append("| %s | %d | %d | %d | %d | %d | %s | %d | %.2f | %.2f | %.2f | %.2f | %s | %s | %s | %s | %s |" % (
            r["block"], r["cin"], r["ce"], r["cout"], r["h"], r["stride"], "yes" if r["residual"] else "no", r["batch"], us["separate"],
            us["separate_again"], spread, max(r["iqr"]["separate"], r["iqr"]["separate_again"]),
            " | ".join("%.2f" % us[f] if f in us else "-" for f in forms), best, "yes (%.2fx)" % (sep_lo / us[best]) if win else "no", static,
            "form%d" % r["autotuned_form"] if r["autotuned_form"] else "separate"))
    k0 = max(rows, key=lambda r: len(r["kernel"]))["kernel"]
    out += ["", "%d of %d rows are won by a form of the one launch; %d of them by at least the margin." % (wins, len(rows), named), "",
            "Forms: " + ", ".join("%s = `%s`" % (f, k0[f]) for f in forms if f in k0) + ".", ""]
    if rule:
        out += ["Rows of `ir_measured_wins` these figures justify (cin, ce, cout, h, stride, batch, form):", "", "```"] + rule + ["```", ""]
    np_ = os.path.join(out_dir, "nets.json")
    if os.path.exists(np_):
        out += ["## MobileNet-v2 INT8, captured and replayed", "",
                "`plain` is the net without flag 32768 - what the parent commit builds for this model - measured in the same process; five",
                "replay timings per configuration (ms per pass, the configurations alternating), launches per pass, and the number of sites that",
                "run the one launch. `inverted_static` is what `ir_static_form` selects for this net, `inverted_autotuned` what",
                "`saber_hip_net_autotune` keeps. (`blocks` and `nets` are separate steps: the rule was written from the table above, then `nets`",
                "was run with it. Two nets with the same selection differ by up to 2 % from one build to the next: compare within a run.)", "",
                "| batch | configuration | ms / pass (five runs) | median | launches | sites on |", "|---|---|---|---|---|---|"]
        for r in json.load(open(np_)):
            for key in ("plain_static", "inverted_static", "plain_autotuned", "inverted_autotuned"):
                out.append("| %d | %s | %s | %.4f | %d | %d |" % (r["batch"], key, " / ".join("%.4f" % v for v in r["ms"][key]), float(np.median(r["ms"][key])),
                                                               r["launches"][key], len(r["sites_on"][key])))
        out.append("")
        fr = [r for r in json.load(open(np_)) if "fp32_ms" in r]
        if fr:
            out += ["## Context: MobileNet-v2 FP32", "",
                    "The reference's benchmark table lists `mobilenetv2` FP32 on a Xeon E5-2650 v4, 8 threads (benchmark/README.md there): 3.785 / 7.246 /",
                    "13.764 / 28.409 ms at batch 1 / 2 / 4 / 8 (Intel Caffe: 23.0 / 65.9 / 85.4 / 131.7 ms), and no INT8 figure. Different hardware: context,",
                    "not a comparison. This project's FP32 net of the same layer list (seeded weights, ReLU), static selection, captured and replayed:", "",
                    "| batch | ms / pass (three runs) | launches |", "|---|---|---|"]
            out += ["| %d | %s | %d |" % (r["batch"], " / ".join("%.4f" % v for v in r["fp32_ms"]), r["fp32_launches"]) for r in fr]
            out.append("")
    open(os.path.join(out_dir, "README.md"), "w").write("\n".join(out))
    print("\n".join(out))
    return 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("step", choices=["blocks", "nets", "table"])
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "ir"))
    a = ap.parse_args()
    sys.exit({"blocks": lambda: blocks(a.out), "nets": lambda: nets(a.out), "table": lambda: table(a.out)}[a.step]() or 0)
