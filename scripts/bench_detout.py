"""The two DetectionOutput forms (anakin_amd/csrc/detout.hip) against each other on four detector rows at batch 1 and 8.

  python scripts/bench_detout.py shapes [--out DIR]   every row x batch, both forms, warm and as the node of a replayed graph, and the copies
                                                      the reference's host route needs -> DIR/shapes.json
  python scripts/bench_detout.py table  [--out DIR]   DIR/shapes.json -> DIR/table.md, the table of DIR/README.md (no GPU needed); exit status 1 when the static rule
                                                      (detout_static_form: api_detout.hip) does not hold on the rows
  python scripts/bench_detout.py check  [--out DIR]   every row x batch once per form, nothing timed: y and count `==`
                                                      tests/detout_util.detout_ref (computed on the CPU) -> DIR/check.txt; exit status 1
                                                      when a line fails

Protocol (scripts/bench_resize.py's): ONE process, the candidates alternating, after a warm-up, device events.
  warm   WARM_LAUNCHES back-to-back runs per window, median of WARM_REPS windows per candidate, per run (a run is two launches);
  graph  the op as the only node pair of a captured one-op list (S.Net), GRAPH_LAUNCHES replays per window, median of WARM_REPS windows.
Form 0 is timed twice, as two separate candidates: the difference is the run-to-run spread.
copies: the device-to-host copies of the decoded boxes (n * P * 4 floats) and the scores (n * P * C floats) and the host-to-device copy of
n * keep_top_k rows, pinned host memory, one stream, synchronised once - what the reference's GPU route moves AROUND its host nms_detect. A
lower bound of that route: no NMS in it.
Inputs: priors on the detector's grids, CENTER_SIZE predictions, scores from a softmax of seeded logits with a favoured background class.
Each step is one process with its own exit status: run it under `timeout`."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

# (what, P, C); nms_top_k 400, keep_top_k 200, conf_thresh 0.01, nms_thresh 0.45, background 0
ROWS = [("MobileNet-SSD", 1917, 21), ("SSD300", 8732, 21), ("SSD300 on 81 classes", 8732, 81), ("SSD512", 24564, 21)]
BATCHES = (1, 8)
NMS_K, KEEP, CONF_T, NMS_T = 400, 200, 0.01, 0.45
WARM_REPS, WARM_LAUNCHES, GRAPH_LAUNCHES = 9, 10, 10
NAMES = ["detout_direct_f32", "detout_mask_f32"]
MARGIN = 0.9      # form 1 is named only where it is ahead of form 0 by at least a tenth


def case(n, p, c):
    from tests import detout_util as DU
    return DU.case(n, c, p, code=DU.CENTER_SIZE, bg=0, keep=KEEP, nms_k=NMS_K, conf_t=CONF_T, nms_t=NMS_T)


def make(n, p, c, seed):
    """loc [n, p * 4], conf [n, p, c] (a softmax), prior [2, p * 4]"""
    rng = np.random.default_rng(seed)
    ctr = rng.uniform(0.05, 0.95, (p, 2))
    half = rng.uniform(0.02, 0.25, (p, 2))
    prior = np.stack([np.concatenate([ctr - half, ctr + half], 1).reshape(-1), np.tile(np.array([0.1, 0.1, 0.2, 0.2]), p)]).astype(np.float32)
    loc = rng.normal(0, 1.0, (n, p * 4)).astype(np.float32)
    logit = rng.normal(0, 2.0, (n, p, c)).astype(np.float32)
    logit[..., 0] += np.float32(8.0)
    e = np.exp(logit - logit.max(-1, keepdims=True))
    conf = (e / e.sum(-1, keepdims=True)).astype(np.float32)
    return loc, conf, prior


def _op(n, p, c):
    from anakin_amd import saber as S
    from tests import detout_util as DU
    return S.SaberDetectionOutput(n, c, p, KEEP, NMS_K, CONF_T, NMS_T, 0, DU.CENTER_SIZE, False, True, 1.0)


def shapes(out_dir):
    import torch
    from anakin_amd import lib as L
    from anakin_amd import saber as S
    L.require_device()
    torch.cuda.set_stream(torch.cuda.Stream())
    rows = []
    for (what, p, c) in ROWS:
        for n in BATCHES:
            loc, conf, prior = make(n, p, c, 7)
            op = _op(n, p, c)
            static = op.tile()
            ld, cd, pd = (torch.from_numpy(a).cuda() for a in (loc, conf, prior))
            y, cnt = op.new_outputs()
            cands = [("form0", 0), ("form0_again", 0), ("form1", 1)]
            for kk, f in cands:
                op.set_tile(f)
                for _ in range(3):
                    op.run(ld, cd, pd, y, cnt)
            torch.cuda.synchronize()
            share = float((conf[..., 1:] > CONF_T).mean())
            kept = int(cnt.cpu()[0])
            ev = []
            for _ in range(WARM_REPS):
                for kk, f in cands:
                    op.set_tile(f)
                    op.run(ld, cd, pd, y, cnt)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(WARM_LAUNCHES):
                        op.run(ld, cd, pd, y, cnt)
                    e1.record()
                    ev.append((kk, e0, e1))
            torch.cuda.synchronize()
            warm = {kk: [] for kk, _ in cands}
            for kk, e0, e1 in ev:
                warm[kk].append(e0.elapsed_time(e1) * 1000.0 / WARM_LAUNCHES)
            # the op as a captured one-op list
            net = S.Net()
            for nm, shape in (("loc", loc.shape), ("conf", conf.shape), ("prior", prior.shape), ("y", (n * KEEP, 7)), ("count", (1 + n,))):
                net.add_tensor(nm, shape, L.F32)
            gop = _op(n, p, c)
            net.add_detout(gop, "loc", "conf", "prior", "y", "count")
            net.finalize()
            for nm, t in (("loc", ld), ("conf", cd), ("prior", pd)):
                net.tensor(nm).copy_(t)
            graph = {kk: [] for kk, _ in cands}
            for _ in range(WARM_REPS):
                for kk, f in cands:
                    net.set_choices([(20 << 16) | f])
                    net.capture()
                    net.replay()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(GRAPH_LAUNCHES):
                        net.replay()
                    e1.record()
                    torch.cuda.synchronize()
                    graph[kk].append(e0.elapsed_time(e1) * 1000.0 / GRAPH_LAUNCHES)
            # the copies around the reference's host NMS
            hb = torch.empty((n, p * 4), dtype=torch.float32).pin_memory()
            hc = torch.empty((n, p, c), dtype=torch.float32).pin_memory()
            hr = torch.zeros((n * KEEP, 7), dtype=torch.float32).pin_memory()
            copies = []
            for _ in range(WARM_REPS + 2):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                hb.copy_(ld, non_blocking=True)
                hc.copy_(cd, non_blocking=True)
                y.copy_(hr, non_blocking=True)
                e1.record()
                torch.cuda.synchronize()
                copies.append(e0.elapsed_time(e1) * 1000.0)
            row = dict(what=what, p=p, c=c, batch=n, static_form=static, share_above_thresh=share, rows_kept=kept,
                       us_warm={kk: float(np.median(v)) for kk, v in warm.items()}, us_graph={kk: float(np.median(v)) for kk, v in graph.items()},
                       us_copies=float(np.median(copies[2:])))
            rows.append(row)
            print(json.dumps(row), flush=True)
    os.makedirs(out_dir, exist_ok=True)
    json.dump(rows, open(os.path.join(out_dir, "shapes.json"), "w"), indent=1)


def check(out_dir):
    """the rows of shapes.json compared with detout_ref (the timing runs compare nothing): both forms, y and count `==`"""
    import torch
    from anakin_amd import lib as L
    from tests import detout_util as DU
    L.require_device()
    lines, bad = ["# scripts/bench_detout.py check: CENTER_SIZE, nms_top_k %d, keep_top_k %d, conf_thresh %g; both forms once against "
                  "tests/detout_util.py detout_ref" % (NMS_K, KEEP, CONF_T), "# criterion: every byte of y and count equal (the largest relative difference of a box column is printed for a line that fails)"], 0
    for (what, p, c) in ROWS:
        for n in BATCHES:
            loc, conf, prior = make(n, p, c, 7)
            want_y, want_c = DU.detout_ref(case(n, p, c), loc, conf, prior)
            op = _op(n, p, c)
            ld, cd, pd = (torch.from_numpy(a).cuda() for a in (loc, conf, prior))
            for f in op.forms():
                op.set_tile(f)
                y, cnt = op.new_outputs()
                y.fill_(float("nan"))
                cnt.fill_(77)
                op.run(ld, cd, pd, y, cnt)
                torch.cuda.synchronize()
                gy, k = y.cpu().numpy(), int(want_c[0])
                ok = DU.same_bits(cnt.cpu().numpy(), want_c) and DU.same_bits(gy, want_y)
                d = float(np.abs(gy[:k, 3:].astype(np.float64) - want_y[:k, 3:]).max() / np.abs(want_y[:k, 3:]).max()) if k else 0.0
                bad += not ok
                lines.append("%-22s P %5d C %2d batch %d %-18s rows %4d  boxes rel. diff %.3g  %s" % (what, p, c, n, NAMES[f], k, d, "equal" if ok else "DIFFERENT"))
                print(lines[-1], flush=True)
    lines.append("# %d lines, %d failed" % (len(lines) - 2, bad))
    os.makedirs(out_dir, exist_ok=True)
    open(os.path.join(out_dir, "check.txt"), "w").write("\n".join(lines) + "\n")
    return 1 if bad else 0


def table(out_dir):
    rows = json.load(open(os.path.join(out_dir, "shapes.json")))
    out = ["| case | P | C | batch | scores above threshold | rows kept | form 0 warm us | form 0 again | form 1 warm us | 1 / 0 | form 0 graph us | "
           "form 1 graph us | 1 / 0 | copies alone us | static |", "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    broken = 0
    for r in rows:
        w, g = r["us_warm"], r["us_graph"]
        ahead = w["form1"] <= MARGIN * w["form0"] and g["form1"] <= MARGIN * g["form0"]
        broken += (r["static_form"] == 1) != ahead
        out.append("| %s | %d | %d | %d | %.1f %% | %d | %.1f | %.1f | %.1f | %.2f | %.1f | %.1f | %.2f | %.1f | %d%s |" % (
            r["what"], r["p"], r["c"], r["batch"], 100 * r["share_above_thresh"], r["rows_kept"], w["form0"], w["form0_again"], w["form1"],
            w["form1"] / w["form0"], g["form0"], g["form1"], g["form1"] / g["form0"], r["us_copies"], r["static_form"],
            "" if (r["static_form"] == 1) == ahead else " (rule broken)"))
    text = "\n".join(out) + "\n"
    print(text)
    open(os.path.join(out_dir, "table.md"), "w").write(text)
    return 1 if broken else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("step", choices=["shapes", "table", "check"])
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "detout"))
    a = ap.parse_args()
    sys.exit({"shapes": shapes, "table": table, "check": check}[a.step](a.out) or 0)
