"""Writes tests/golden/fc_softmax_tail.npz: what the fc + Softmax launch (saber_hip_fc_run_softmax) of a BUILT TREE writes as prob for the
seeded inputs of tests/tail_util.py's FC_CASES. Run ONCE on a GPU against a built copy of the commit whose bits are to be pinned (it was:
the parent of the commit that moved the launch's tail from four waves to eight); the file is then committed unchanged and
tests/test_gpu_tail.py compares every later tree with it, bit for bit.

    python scripts/record_fc_softmax_golden.py [output.npz] [root of the built tree whose library runs; default: this tree]

Per case the file holds `<key>/prob` (float32 [M][N]) and `<key>/inputs` (crc32 of the weights, scales, bias and input)."""
import importlib.util
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOT = os.path.abspath(sys.argv[2]) if len(sys.argv) > 2 else HERE
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from anakin_amd import lib as L  # noqa: E402
from oracle import oracle as O  # noqa: E402

spec = importlib.util.spec_from_file_location("tail_util", os.path.join(HERE, "tests", "tail_util.py"))
T = importlib.util.module_from_spec(spec)
spec.loader.exec_module(T)


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else T.GOLDEN
    L.require_device()
    print("library of", os.path.dirname(os.path.abspath(L.__file__)))
    data = {}
    for case in T.FC_CASES:
        M, K, N, dt = case
        wq, ws, b, out_scale, xs = T.fc_case(case)
        fc = T.fc_op(case, wq, ws, b, out_scale)
        y = torch.empty((M, N), dtype=torch.float32, device="cuda")
        p = torch.empty((M, N), dtype=torch.float32, device="cuda")
        runs = []
        for rep in range(3):          # the same bits on every launch, or nothing is recorded
            y.fill_(7.0)
            p.fill_(-1.0)
            fc.dispatch_softmax(torch.from_numpy(xs[0]).cuda(), y, p)
            torch.cuda.synchronize()
            runs.append(p.cpu().numpy().copy())
        assert all(np.array_equal(r.view(np.uint32), runs[0].view(np.uint32)) for r in runs), case
        want = T.fc_oracle(case, wq, ws, b, out_scale, xs[0])
        assert np.array_equal(y.cpu().numpy(), want), case
        sm = O.softmax_f32(want)
        assert np.abs(runs[0] - sm).max() <= 1e-4 * sm.max(), case
        key = T.fc_key(case)
        data[key + "/prob"] = runs[0]
        data[key + "/inputs"] = T.fingerprint(wq, ws, b, xs[0])
        print("%s: %s, %d values" % (key, fc.algo(), runs[0].size))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    np.savez(out, **data)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
