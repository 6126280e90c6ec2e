"""SqueezeNet v1.1's Fire modules as the executor runs them - squeeze 1x1, expand 1x1, expand 3x3, concat: four launches - and the whole
INT8 net. These are the figures a one-launch Fire kernel has to beat; the library has no such kernel yet, so there are no forms to
compare, only the baseline and what share of it the concat copy is.

  python scripts/bench_fire.py modules [--out DIR]    the 8 Fire modules at 224 x 224 x batch 1 / 8, operands cold in L2
  python scripts/bench_fire.py nets    [--out DIR]    squeezenet_v1_1 INT8, batch 1 / 8, captured and replayed, static and autotuned
  python scripts/bench_fire.py table   [--out DIR]    DIR/modules.json + DIR/nets.json -> DIR/README.md (no GPU needed)

`modules` puts each module into a net of its own, lets saber_hip_net_autotune tune the three convs, and times in ONE process,
alternating, with device events and a 64 MB stream through the L2s between two timed runs (as the autotuner's ColdBench does): the four
launches TWICE, as two candidates - their difference is the run's spread - and the three convs without the concat copy (what a
zero-copy concat, convs writing into channel slices of the wider tensor, would leave).
Both also captured and replayed as one hipGraph per module (no host gap between the launches): the baseline for a one-launch kernel.
Each step is one process with its own exit status: run it under `timeout`."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

REPS = 15
MARGIN = 1.10      # fire_static_form's condition on a winning row: four / form >= MARGIN
FIRE_FLAG = 65536


def fire_modules():
    """(name, C, S, E1, E3, H, input is u8) of the 8 Fire modules at 224 x 224, in network order"""
    from anakin_amd import workloads as W
    spec = W.framework_spec(W.squeezenet_v1_1_spec(), "int8")
    by = {l["name"]: l for l in spec}
    size, out = {"data": 224}, []
    for l in spec:
        if l["kind"] == "conv":
            size[l["name"]] = (size[l["src"]] + 2 * l["pad"] - l["k"]) // l["stride"] + 1
        elif l["kind"] == "pool":
            size[l["name"]] = -(-(size[l["src"]] - l["win"]) // l["stride"]) + 1
        elif l["kind"] == "concat":
            size[l["name"]] = size[l["srcs"][0]]
            f = l["name"][:-len("_concat")]
            sq = by[f + "_squeeze1x1"]
            src = by[sq["src"]]
            u8 = src["kind"] == "concat" or (src["kind"] == "pool" and by[src["src"]]["kind"] == "concat")
            out.append((f, sq["cin"], sq["cout"], by[f + "_expand1x1"]["cout"], by[f + "_expand3x3"]["cout"], size[sq["name"]], u8))
    assert len(out) == 8
    return out


def _module_net(S, L, rng, n, c, s, e1, e3, h, u8):
    lay = dict(in_layout=L.NHWC, out_layout=L.NHWC)
    idt = L.U8 if u8 else L.S8

    def conv(cin, cout, k, in_dt):
        w = (rng.standard_normal((cout, cin, k, k)) / np.sqrt(cin * k * k)).astype(np.float32)
        b = rng.standard_normal(cout).astype(np.float32) * 0.1
        return S.SaberConv2D(True).init((n, cin, h, h), S.ConvParam(w, b, 1, (k // 2,) * 2, (1, 1), (1, 1), True), in_dt, L.U8, 0.02, 0.05, **lay)
    ops = [conv(c, s, 1, idt), conv(s, e1, 1, L.U8), conv(s, e3, 3, L.U8)]
    nets_ = []
    for kind in ("four", "convs", 1, 2):      # the module; the same three conv objects (one selection) without the copy; the one launch, per form
        with_concat = kind != "convs"
        net = S.Net()
        net.add_tensor("x", (n, h, h, c), idt)
        net.add_tensor("s", (n, h, h, s), L.U8)
        net.add_tensor("a", (n, h, h, e1), L.U8)
        net.add_tensor("b", (n, h, h, e3), L.U8)
        net.add_conv(ops[0], "x", "s")
        net.add_conv(ops[1], "s", "a")
        net.add_conv(ops[2], "s", "b")
        if with_concat:
            net.add_tensor("y", (n, h, h, e1 + e3), L.U8)
            net.add_concat(["a", "b"], "y")
        net.optimize(15)
        if isinstance(kind, int):
            assert net.optimize(FIRE_FLAG) == 1
            word = net.choices()[0] & ~(15 << 24)
            if L.load().saber_hip_net_set_choice(net.h, 0, word | (kind << 24)) != 0:
                nets_.append(None)      # no such form for this module
                continue
        net.finalize()
        assert net.num_ops() == 3 + with_concat and net.num_launches() == (1 if isinstance(kind, int) else 3 + with_concat)
        nets_.append(net)
    return nets_


def modules(out_dir):
    import torch
    from anakin_amd import lib as L
    from anakin_amd import saber as S
    L.require_device()
    torch.cuda.set_stream(torch.cuda.Stream())
    rng = np.random.default_rng(0)
    flush = torch.ones(16 << 20, dtype=torch.float32, device="cuda")      # 64 MB
    sink = torch.zeros(1, dtype=torch.float32, device="cuda")
    rows = []
    for (tag, c, s, e1, e3, h, u8) in fire_modules():
        for n in (1, 8):
            net, net3, nf1, nf2 = _module_net(S, L, rng, n, c, s, e1, e3, h, u8)
            fnets = {"form1": nf1, "form2": nf2}
            x = net.tensor("x")
            x.copy_((torch.rand(x.shape, device="cuda") * (255 if u8 else 200) - (0 if u8 else 100)).to(x.dtype))
            net3.tensor("x").copy_(x)
            for fn in fnets.values():
                if fn is not None:
                    fn.tensor("x").copy_(x)
            net.run()
            net.autotune(iters=7)      # (the conv objects are shared: net3 runs the same selection)
            cands = [("four", 4), ("four_again", 4), ("convs", 3), ("four_graph", -4), ("four_graph_again", -4), ("convs_graph", -3)]
            cands += [(k, 0) for k, fn in fnets.items() if fn is not None] + [(k + "_graph", -1) for k, fn in fnets.items() if fn is not None]
            t = {key: [] for key, _ in cands}
            for _ in range(3):
                net.run()
                net3.run()
            net.capture()
            net3.capture()
            for fn in fnets.values():
                if fn is not None:
                    for _ in range(3):
                        fn.run()
                    fn.capture()
            torch.cuda.synchronize()
            ev = [(key, torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(REPS) for key, _ in cands]
            i = 0
            for _ in range(REPS):
                for key, nops in cands:
                    sink.add_(flush.sum())
                    ev[i][1].record()
                    if key.startswith("form"):      # the one launch: eager, or as a one-node graph
                        fn = fnets[key[:5]]
                        fn.replay() if nops < 0 else fn.run()
                    elif nops < 0:      # the whole module as one replayed hipGraph: no host gaps between the launches
                        (net if nops == -4 else net3).replay()
                    for op in range(max(nops, 0)):
                        net.run_op(op)
                    ev[i][2].record()
                    i += 1
            torch.cuda.synchronize()
            for key, e0, e1_ in ev:
                t[key].append(e0.elapsed_time(e1_) * 1000.0)
            us = {key: float(np.median(v)) for key, v in t.items()}
            iqr = {key: float(np.percentile(v, 75) - np.percentile(v, 25)) for key, v in t.items()}
            row = dict(module=tag, c=c, s=s, e1=e1, e3=e3, h=h, x="u8" if u8 else "s8", batch=n, us=us, iqr=iqr,
                       kernel=[net.op_name(i) for i in range(4)], bytes=[net.op_work(i)[0] for i in range(4)],
                       form_kernel={k: fn.op_name(0)[5:] for k, fn in fnets.items() if fn is not None})
            rows.append(row)
            print(json.dumps(row), flush=True)
    os.makedirs(out_dir, exist_ok=True)
    json.dump(rows, open(os.path.join(out_dir, "modules.json"), "w"), indent=1)


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
    model = W.build_model("squeezenet_v1_1")
    fw = W.framework_model(model, "int8")
    rows = []
    for batch in (1, 8):
        x = W.make_input(batch)
        scales = W.calibrate(model, x)
        net = W.build_int8_net(fw, dict(scales), batch)
        net.tensor("data").copy_(torch.from_numpy(x).cuda())
        net.run()
        static = net.choices()
        net.autotune(iters=7)
        tuned = net.choices()
        ms = {}
        for rep in range(5):      # five times, alternating: the spread between the rounds is the noise
            for sel, ch in (("static", static), ("autotuned", tuned)):
                net.set_choices(ch)
                ms.setdefault(sel, []).append(_replay_ms(net))
        fnet = W.build_int8_net(fw, dict(scales), batch, fire=True)
        fnet.tensor("data").copy_(torch.from_numpy(x).cuda())
        fnet.run()
        fstatic = fnet.choices()
        fnet.autotune(iters=7)
        ftuned = fnet.choices()
        forced = [(c & ~(15 << 24)) | (1 << 24) if (c >> 30) & 3 == 2 else c for c in ftuned]
        sites_on = {}
        for rep in range(5):
            for sel, ch in (("fire_static", fstatic), ("fire_autotuned", ftuned), ("fire_all_form1", forced)):
                fnet.set_choices(ch)
                ms.setdefault(sel, []).append(_replay_ms(fnet))
                sites_on[sel] = (sum(1 for c in fnet.choices() if (c >> 30) & 3 == 2 and (c >> 24) & 15), fnet.num_launches())
            for sel, ch in (("static", static), ("autotuned", tuned)):      # (the plain net again, alternating with the flagged one)
                net.set_choices(ch)
                ms.setdefault(sel + "_again", []).append(_replay_ms(net))
        net.set_choices(tuned)
        share = net.time_pass(20)
        cat = sum(t for i, t in enumerate(share) if net.op_name(i).startswith("concat"))
        f32 = W.build_fp32_net(model, batch)
        f32.tensor("data").copy_(torch.from_numpy(x).cuda())
        f32.run()
        row = dict(model="squeezenet_v1_1", precision="int8", batch=batch, ms=ms, launches=net.num_launches(), ops=net.num_ops(),
                   concat_share_of_eager_pass=cat / sum(share), fire_sites_on_and_launches=sites_on, fp32_ms=[_replay_ms(f32) for _ in range(3)], fp32_launches=f32.num_launches())
        rows.append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(out_dir, exist_ok=True)
    json.dump(rows, open(os.path.join(out_dir, "nets.json"), "w"), indent=1)


def table(out_dir):
    rows = json.load(open(os.path.join(out_dir, "modules.json")))
    forms = ["form1", "form2"]
    out = ["# Fire module launch: `conv_fire.hip` against the four tuned launches it replaces", "",
           "Written by `scripts/bench_fire.py table` from `modules.json` / `nets.json` (MI355X, cold-L2 medians of %d runs per candidate," % REPS,
           "candidates alternating in one process; every conv with bias and relu -> u8). `four` is squeeze 1x1 + expand 1x1 + expand 3x3 + concat,",
           "all tuned by `saber_hip_net_autotune` - what the parent path runs for these ops - timed twice: `spread` is the difference of the two",
           "medians, `iqr` the larger interquartile range of the two. `convs` is the three convs without the concat copy (what a zero-copy",
           "concat would leave). `formN`: the one launch. These columns are enqueued eagerly: `four` holds the gaps between its launches.",
           "`g.`: the same candidates each captured as a hipGraph of its own and replayed (a replay carries the graph launch's start-up, the same",
           "for every candidate). A form `wins` a row where it is below BOTH timings of the four launches by more than the spread. `static` is",
           "what `fire_static_form` (api_fire.hip) does with the row: the best form where the row is won by at least %d %% eagerly AND replayed" % round((MARGIN - 1) * 100),
           "(`formN`), else 0 = four launches (`off: under the margin` / `off`).", "",
           "| module | C | S | E1 + E3 | H | x | batch | four us | again | spread | iqr | convs us | " + " | ".join("%s us" % f for f in forms) +
           " | best | wins | g.four us | again | g.convs us | " + " | ".join("g.%s us" % f for f in forms) + " | g.best ratio | static |",
           "|---|---|---|---|---|---|---|---|---|---|---|---|" + "---|" * len(forms) + "---|---|---|---|---|" + "---|" * len(forms) + "---|---|"]
    wins = named = 0
    rule = []
    for r in rows:
        us = r["us"]
        lo, spread = min(us["four"], us["four_again"]), abs(us["four"] - us["four_again"])
        glo = min(us["four_graph"], us["four_graph_again"])
        have = [f for f in forms if f in us]
        best = min(have, key=lambda f: us[f])
        win = us[best] < lo - spread
        wins += win
        gratio = glo / us[best + "_graph"]
        static = best if win and lo / us[best] >= MARGIN and gratio >= MARGIN else ("off: under the margin" if win else "off")
        if static == best:
            named += 1
            rule.append("    {%d, %d, %d, %d, %d, %d, %s},      // %s: %.1f against %.1f / %.1f (%.2fx; replayed %.2fx)" % (
                r["c"], r["s"], r["e1"], r["e3"], r["h"], r["batch"], best[4:], r["module"], us[best], us["four"], us["four_again"], lo / us[best], gratio))
        out.append("| %s | %d | %d | %d + %d | %d | %s | %d | %.2f | %.2f | %.2f | %.2f | %.2f | %s | %s | %s | %.2f | %.2f | %.2f | %s | %.2fx | %s |" % (
            r["module"], r["c"], r["s"], r["e1"], r["e3"], r["h"], r["x"], r["batch"], us["four"], us["four_again"], spread,
            max(r["iqr"]["four"], r["iqr"]["four_again"]), us["convs"], " | ".join("%.2f" % us[f] if f in us else "-" for f in forms), best,
            "yes (%.2fx)" % (lo / us[best]) if win else "no", us["four_graph"], us["four_graph_again"], us["convs_graph"],
            " | ".join("%.2f" % us[f + "_graph"] if f + "_graph" in us else "-" for f in forms), gratio, static))
    k0 = rows[0].get("form_kernel", {})
    out += ["", "%d of %d rows are won by a form of the one launch; %d of them by at least the margin in both comparisons." % (wins, len(rows), named), "",
            "Forms: " + ", ".join("%s = `%s`" % (f, k0[f]) for f in forms if f in k0) + ". The launch wins where the image is large (55 x 55, 27 x 27: many",
            "workgroups, a narrow inner edge) and loses at 13 x 13 with C = 384 / 512, where 4 - 7 workgroups per image each read the whole of the",
            "expand weights and run nine 64-deep k-steps per tap-padded 3x3 for S = 48 / 64.", ""]
    if rule:
        out += ["Rows of `fire_measured_wins` these figures justify (c, s, e1, e3, h, batch, form):", "", "```"] + rule + ["```", ""]
    np_ = os.path.join(out_dir, "nets.json")
    if os.path.exists(np_):
        out += ["## squeezenet_v1_1 INT8, captured and replayed", "",
                "`static` / `autotuned`: the net without flag 65536 - what the parent path builds - in the same process (`_again`: timed once more,",
                "alternating with the flagged net). `fire_static`: `build_int8_net(fire=True)` with what `fire_static_form` selects (`modules` and",
                "`nets` are separate steps: the rule was written from the table above, then `nets` was run with it); `fire_autotuned`: what",
                "`saber_hip_net_autotune` keeps; `fire_all_form1`: every site forced on. Five replay timings each (ms per pass).", "",
                "| batch | selection | ms / pass (five runs) | median | sites on | launches |", "|---|---|---|---|---|---|"]
        nr = json.load(open(np_))
        for r in nr:
            for key in ("static", "static_again", "fire_static", "autotuned", "autotuned_again", "fire_autotuned", "fire_all_form1"):
                on, ln = r["fire_sites_on_and_launches"].get(key, (0, r["launches"]))
                out.append("| %d | %s | %s | %.4f | %d | %d |" % (r["batch"], key, " / ".join("%.4f" % v for v in r["ms"][key]), float(np.median(r["ms"][key])), on, ln))
        out += ["", "FP32 net of the same layer list, static selection, captured and replayed:", "", "| batch | ms / pass (three runs) | launches |", "|---|---|---|"]
        out += ["| %d | %s | %d |" % (r["batch"], " / ".join("%.4f" % v for v in r["fp32_ms"]), r["fp32_launches"]) for r in nr]
        out.append("")
    open(os.path.join(out_dir, "README.md"), "w").write("\n".join(out))
    print("\n".join(out))
    return 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("step", choices=["modules", "nets", "table"])
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "fire"))
    a = ap.parse_args()
    sys.exit({"modules": lambda: modules(a.out), "nets": lambda: nets(a.out), "table": lambda: table(a.out)}[a.step]() or 0)
