"""Depthwise 3x3 kernels against the direct kernel they replace, and MobileNet-v1 with and without them.

  python scripts/bench_dw.py shapes [--out DIR]     the nine MobileNet-v1 depthwise shapes x batch 1 / 8 x INT8 (u8 -> u8) / FP32
  python scripts/bench_dw.py nets   [--out DIR]     MobileNet-v1 INT8 / FP32, batch 1 / 8, captured and replayed
  python scripts/bench_dw.py trace                  a few replays of MobileNet-v1 INT8 batch 8 (the program for `rocprofv3 --kernel-trace
                                                    --stats -- python scripts/bench_dw.py trace`)
  python scripts/bench_dw.py table  [--out DIR]     DIR/shapes.json + DIR/nets.json -> DIR/README.md (no GPU needed)

`shapes` times every selectable form of each op in ONE process, alternating between the forms, after a warm-up, with device events
and the operands cold in L2 - between two timed launches a 64 MB buffer is streamed through the L2s, as the autotuner's ColdBench
does (the 256 MB Infinity Cache keeps the operands). Form 0 (the direct kernel) is timed twice, as two separate candidates: the
difference is the run-to-run spread the selection rule is judged against. Bytes are saber_hip_net_op_work's algorithmic bytes;
the share is of the 8 TB/s HBM peak - at these sizes the bound is often the launch itself (5 - 6.5 us, profiles/r06/int8_b8_floor.md).
Each step is one process with its own exit status: run it under `timeout`."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

SHAPES = [(32, 112, 1), (64, 112, 2), (128, 56, 1), (128, 56, 2), (256, 28, 1), (256, 28, 2), (512, 14, 1), (512, 14, 2), (1024, 7, 1)]
HBM_PEAK = 8.0e12
REPS = 15


def _forms(lib, conv):
    v, out = 1, []
    while lib.saber_hip_conv2d_set_tile(conv.h, (16 << 16) | v) == 0:
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
    for int8 in (True, False):
        for (c, h, s) in SHAPES:
            for n in (1, 8):
                w = (rng.standard_normal((c, 1, 3, 3)) * 0.4).astype(np.float32)
                b = rng.standard_normal(c).astype(np.float32)
                prm = S.ConvParam(w, b, c, (1, 1), (s, s), (1, 1), True)
                dt = L.U8 if int8 else L.F32
                conv = S.SaberConv2D(int8).init((n, c, h, h), prm, dt, dt, 0.02, 0.05, in_layout=L.NHWC, out_layout=L.NHWC)
                static = lib.saber_hip_conv2d_get_tile(conv.h) & 0xff
                ho = conv.out_hw[0]
                net = S.Net()
                net.add_tensor("x", (n, h, h, c), dt)
                net.add_tensor("y", (n, ho, ho, c), dt)
                net.add_conv(conv, "x", "y")
                net.finalize()
                nbytes, flops = net.op_work(0)
                x, y = net.tensor("x"), net.tensor("y")
                x.copy_((torch.rand(x.shape, device="cuda") * 200).to(x.dtype))
                cands = [("form0", 0), ("form0_again", 0)] + [("form%d" % v, v) for v in _forms(lib, conv)]
                names, t = {}, {k: [] for k, _ in cands}
                for k, v in cands:      # warm-up: code and kernel arguments of every form
                    conv.set_tile((16 << 16) | v)
                    names[k] = conv.algo()
                    for _ in range(3):
                        conv.dispatch(x, y)
                torch.cuda.synchronize()
                ev = [(k, torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(REPS) for k, _ in cands]
                i = 0
                for _ in range(REPS):
                    for k, v in cands:
                        conv.set_tile((16 << 16) | v)
                        sink.add_(flush.sum())
                        ev[i][1].record()
                        conv.dispatch(x, y)
                        ev[i][2].record()
                        i += 1
                torch.cuda.synchronize()
                for k, e0, e1 in ev:
                    t[k].append(e0.elapsed_time(e1) * 1000.0)
                us = {k: float(np.median(v)) for k, v in t.items()}
                row = dict(dtype="int8" if int8 else "fp32", c=c, h=h, stride=s, batch=n, bytes=nbytes, flops=flops, static_form=static,
                           us=us, kernel=names, hbm_share={k: nbytes / (v * 1e-6) / HBM_PEAK for k, v in us.items()})
                rows.append(row)
                print(json.dumps(row), flush=True)
    os.makedirs(out_dir, exist_ok=True)
    json.dump(rows, open(os.path.join(out_dir, "shapes.json"), "w"), indent=1)


def _mobilenet(precision, batch):
    from anakin_amd import workloads as W
    model = W.build_model("mobilenet_v1")
    if precision == "int8":
        x = W.make_input(batch)
        return W.build_int8_net(W.framework_model(model, "int8"), W.calibrate(model, x), batch), x
    return W.build_fp32_net(model, batch), W.make_input(batch)


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
    L.require_device()
    torch.cuda.set_stream(torch.cuda.Stream())
    rows = []
    for precision in ("int8", "fp32"):
        for batch in (1, 8):
            net, x = _mobilenet(precision, batch)
            net.tensor("data").copy_(torch.from_numpy(x).cuda())
            net.run()
            static = net.choices()
            direct = [(16 << 16) if (c >> 16) & 0xff == 16 else c for c in static]
            ms = {}
            for rep in range(2):      # static, direct, static, direct: the second pair shows the spread
                for label, ch in (("static", static), ("dw_ops_on_form0", direct)):
                    net.set_choices(ch)
                    ms.setdefault(label, []).append(_replay_ms(net))
            net.set_choices(static)
            row = dict(model="mobilenet_v1", precision=precision, batch=batch, launches=net.num_launches(), ops=net.num_ops(), ms=ms,
                       dw_kernels=sorted({net.op_name(i) for i, c in enumerate(static) if (c >> 16) & 0xff == 16}))
            rows.append(row)
            print(json.dumps(row), flush=True)
    os.makedirs(out_dir, exist_ok=True)
    json.dump(rows, open(os.path.join(out_dir, "nets.json"), "w"), indent=1)


def trace():
    import torch
    from anakin_amd import lib as L
    L.require_device()
    torch.cuda.set_stream(torch.cuda.Stream())
    net, x = _mobilenet("int8", 8)
    net.tensor("data").copy_(torch.from_numpy(x).cuda())
    for _ in range(20):
        net.run()
    torch.cuda.synchronize()
    print("trace: 20 eager passes of MobileNet-v1 INT8 batch 8,", net.num_launches(), "launches per pass")


def table(out_dir):
    rows = json.load(open(os.path.join(out_dir, "shapes.json")))
    out = ["# Depthwise 3x3: the forms of `conv_dw3x3.hip` against the direct kernel", "",
           "Written by `scripts/bench_dw.py table` from `shapes.json` / `nets.json` (MI355X, cold-L2 medians of %d launches per form," % REPS,
           "forms alternating in one process). `form0` is `conv_direct_kernel`, timed twice: `spread` is the difference of the two.",
           "`share` is algorithmic bytes / time as a share of the 8 TB/s HBM peak, for the fastest form. `static` is what",
           "`saber_hip_conv2d_create` selects; `ok` says that it is not above form 0 by more than the spread.", "",
           "| dtype | C | H | stride | batch | KB | form0 us | again | spread | " +
           " | ".join("%s us" % k for k in sorted(rows[0]["us"]) if k not in ("form0", "form0_again")) + " | best | share | static | ok |",
           "|---|---|---|---|---|---|---|---|---|" + "---|" * (len(rows[0]["us"]) - 2) + "---|---|---|---|"]
    bad = 0
    for r in rows:
        us = r["us"]
        forms = sorted(k for k in us if k not in ("form0", "form0_again"))
        f0, spread = min(us["form0"], us["form0_again"]), abs(us["form0"] - us["form0_again"])
        best = min(["form0"] + forms, key=lambda k: f0 if k == "form0" else us[k])
        st = "form%d" % r["static_form"]
        st_us = f0 if st == "form0" else us[st]
        ok = st_us <= (us["form0"] + us["form0_again"]) / 2 + spread
        bad += not ok
        out.append("| %s | %d | %d | %d | %d | %.0f | %.2f | %.2f | %.2f | %s | %s | %.1f %% | %s | %s |" % (
            r["dtype"], r["c"], r["h"], r["stride"], r["batch"], r["bytes"] / 1024, us["form0"], us["form0_again"], spread,
            " | ".join("%.2f" % us[k] for k in forms), best, 100 * r["bytes"] / (min(f0, *[us[k] for k in forms]) * 1e-6) / HBM_PEAK, st,
            "yes" if ok else "NO"))
    names = rows[0]["kernel"]
    out += ["", "Kernels: " + ", ".join("%s = `%s`" % (k, names[k]) for k in sorted(names) if k != "form0_again") + " (INT8 row 1).", ""]
    np_ = os.path.join(out_dir, "nets.json")
    if os.path.exists(np_):
        out += ["## MobileNet-v1, captured and replayed", "",
                "| precision | batch | launches | static ms / pass | depthwise ops on form 0, ms / pass | ratio |", "|---|---|---|---|---|---|"]
        for r in json.load(open(np_)):
            a, b = r["ms"]["static"], r["ms"]["dw_ops_on_form0"]
            out.append("| %s | %d | %d | %s | %s | %.2f |" % (r["precision"], r["batch"], r["launches"], " / ".join("%.3f" % v for v in a),
                                                            " / ".join("%.3f" % v for v in b), min(b) / min(a)))
        out.append("")
    open(os.path.join(out_dir, "README.md"), "w").write("\n".join(out))
    print("\n".join(out))
    return 1 if bad else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("step", choices=["shapes", "nets", "trace", "table"])
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "dw3x3"))
    a = ap.parse_args()
    sys.exit({"shapes": lambda: shapes(a.out), "nets": lambda: nets(a.out), "trace": trace, "table": lambda: table(a.out)}[a.step]() or 0)
