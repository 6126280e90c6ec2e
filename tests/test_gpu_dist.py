"""bench.py's N > 1 control flow on ONE GPU: two ranks launched by torch.distributed.run share cuda:0
(BENCH_SHARE_GPU=1) and exchange their logits through gloo (BENCH_DIST_BACKEND=gloo) - mode agreement across ranks,
the asynchronous double-buffered logits gather, barrier + max-over-ranks timing and the whole-job aggregate all run
exactly as they do with one GPU per rank over RCCL (which needs a multi-GPU node the driver owns)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_bench_two_ranks_share_one_gpu():
    env = dict(os.environ)
    env.update(BENCH_DIST_BACKEND="gloo", BENCH_SHARE_GPU="1", MASTER_ADDR="127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29533", os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "20", "--warmup", "3",
           "--no-cpu-baseline", "--no-b1"]
    p = subprocess.run(cmd, capture_output=True, text=True, env=env, cwd=ROOT, timeout=900)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]          # rank 0 prints ONE line
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["scaling"] == "weak" and out["config"]["global_batch"] == 16
    assert out["value"] > 0 and abs(out["value"] - 16 * 1000.0 / out["ms_per_step"]) < 0.02 * out["value"]
    assert out["config"]["parallelism"] == "batch-shard x2"


@pytest.mark.gpu
def test_bench_four_ranks_share_one_gpu_and_report_the_per_request_exchange():
    """Four ranks (round-4 verdict item 8) on the one GPU of the box: nets declared SABER_HIP_NET_SHARED_DEVICE (no stage launch / no
    cooperating chains: four processes' kernels interleave on the CUs), logits through gloo; the line carries both exchange cadences -
    amortised over --gather-every steps (the headline) and per request (config.gather.per_request) - and zero cooperative fallbacks."""
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    env.update(BENCH_DIST_BACKEND="gloo", BENCH_SHARE_GPU="1")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4", "--steps", "40", "--warmup", "5", "--full",
                        "--no-cpu-baseline", "--no-b1"], capture_output=True, text=True, env=env, cwd=ROOT, timeout=1200)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    out = json.loads(lines[0])
    cfg = out["config"]
    assert out["n_gpus"] == 4 and cfg["global_batch"] == 32 and cfg["parallelism"] == "batch-shard x4"
    assert cfg["shared_device"] is True and cfg["coop_fallbacks"] == 0 and cfg["coop_fallback"] is False
    assert cfg["rccl_ranks"] == 0 and cfg["dist_backend"] == "gloo"
    g = cfg["gather"]
    assert g["every_steps"] == 16 and g["per_request"]["every_steps"] == 1 and g["per_request"]["ms_per_step"] > 0
    print("4 ranks sharing the GPU: %.4f ms/step amortised gather, %.4f ms/step with a gather per request"
          % (out["ms_per_step"], g["per_request"]["ms_per_step"]))


@pytest.mark.gpu
def test_bench_gpus_2_spawns_its_own_ranks_and_the_gather_is_cheap():
    """`python bench.py --gpus 2` called PLAINLY (no torchrun): the script re-executes itself under torch.distributed.run,
    shards the batch over two ranks (here sharing the one GPU of the test box, logits through gloo), asserts n_gpus == --gpus
    and prints one line. What the exchange costs is isolated by running the same two ranks once more WITHOUT it
    (BENCH_NO_GATHER=1): two PROCESSES time-slicing one GPU are slow for reasons that have nothing to do with the path (no
    concurrent contexts), so the criterion is gather-on <= 1.15 x gather-off, and the host time of one gather call is reported."""
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    common = ["--steps", "60", "--warmup", "5", "--no-cpu-baseline", "--no-b1"]

    def run(extra_env, gpus):
        e = dict(env, **extra_env)
        p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + (["--gpus", str(gpus)] if gpus > 1 else []) + common,
                           capture_output=True, text=True, env=e, cwd=ROOT, timeout=900)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
        lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1, p.stdout[-2000:]
        return json.loads(lines[0])
    o1 = run({}, 1)
    share = dict(BENCH_DIST_BACKEND="gloo", BENCH_SHARE_GPU="1")
    o2 = run(share, 2)
    o2n = run(dict(share, BENCH_NO_GATHER="1"), 2)
    assert o2["n_gpus"] == 2 and o2["config"]["global_batch"] == 16
    # the dry run exchanges through gloo: no RCCL communicator exists, and the line must say so
    assert o2["config"]["dist_backend"] == "gloo" and o2["config"]["rccl_ranks"] == 0
    assert o2["config"]["gather"]["every_steps"] == 16 and o2["config"]["gather"]["host_us_per_step"] > 0
    assert o2n["config"]["gather"] is None
    print("1 rank: %.4f ms/step; 2 ranks sharing the GPU: %.4f ms/step with the logits gather, %.4f without (x%.3f); "
          "gather host time %.1f us per step" % (o1["ms_per_step"], o2["ms_per_step"], o2n["ms_per_step"],
                                                  o2["ms_per_step"] / o2n["ms_per_step"], o2["config"]["gather"]["host_us_per_step"]))
    assert o2["ms_per_step"] <= 1.15 * o2n["ms_per_step"], (o2["ms_per_step"], o2n["ms_per_step"])
    # a wrong world size is refused instead of silently running one rank
    bad = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--no-cpu-baseline", "--no-b1"],
                         capture_output=True, text=True, env=dict(env, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0"), cwd=ROOT, timeout=600)
    assert bad.returncode != 0 and "--gpus 2 but WORLD_SIZE is 1" in (bad.stdout + bad.stderr)


RCCL_ONE_RANK = r'''
import os, sys
import torch
import torch.distributed as dist
sys.path.insert(0, os.environ["REPO_ROOT"])
from anakin_amd import shard
torch.cuda.set_device(0)
dist.init_process_group("nccl", init_method="tcp://127.0.0.1:%s" % os.environ["PORT"], world_size=1, rank=0, device_id=torch.device("cuda", 0))
assert dist.get_backend() == "nccl"
g = torch.Generator().manual_seed(5)
steps = [torch.randn(8, 1000, generator=g).cuda() for _ in range(40)]
# the blocking gather (world 1 goes through all_gather_into_tensor when asked to: call the collective itself)
out = torch.empty_like(steps[0])
dist.all_gather_into_tensor(out, steps[0])
torch.cuda.synchronize()
assert torch.equal(out, steps[0])
# per-step asynchronous gather (double-buffered), on a side stream like bench.py's compute stream
st = torch.cuda.Stream()
with torch.cuda.stream(st):
    ag = shard.AsyncLogitGather(steps[0], 1)
    for i, x in enumerate(steps):
        ag.step(x)
        if i:
            ag_prev = ag.latest()
            assert ag_prev is not None
    ag.flush()
    st.synchronize()
    assert torch.equal(ag.latest(), steps[-1])
    # the amortised gather: one collective per 16 steps + the remainder ring (40 = 2 x 16 + 8)
    bg = shard.BatchedLogitGather(steps[0], 1, every=16)
    seen = []
    for i, x in enumerate(steps):
        bg.step(x)
        if (i + 1) % 16 == 0:
            bg.flush()
            st.synchronize()
            seen.append(bg.latest().clone())
    bg.finish()
    st.synchronize()
    seen.append(bg.latest().clone())
assert bg.gathers == 3 and [tuple(s.shape) for s in seen] == [(1, 16, 8, 1000), (1, 16, 8, 1000), (1, 8, 8, 1000)]
flat = torch.cat([s[0] for s in seen], 0)
assert torch.equal(flat, torch.stack(steps, 0))
dist.barrier()
dist.destroy_process_group()
print("rccl one rank ok: backend nccl, %d gathers, every logit bit-identical" % bg.gathers)
'''


@pytest.mark.gpu
def test_rccl_all_gather_paths_run_on_the_device_with_one_rank(tmp_path):
    """No multi-GPU node has been available to this build, and two ranks cannot share a device under RCCL (the N > 1 dry runs above go through
    gloo). What CAN run on one MI355X: an RCCL communicator of ONE rank - `ncclCommInitRank`, `ncclAllGather` on device tensors from a side
    stream, asynchronous work handles - through exactly the code of anakin_amd/shard.py that `bench.py --gpus N` uses with the nccl backend
    (the blocking gather, the per-step double-buffered gather, the amortised ring with its remainder): every gathered logit bit-identical."""
    script = tmp_path / "rccl_one_rank.py"
    script.write_text(RCCL_ONE_RANK)
    import socket
    with socket.socket() as so:          # a port nobody holds (two suites on one host must not meet on a fixed one)
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    env = dict(os.environ, REPO_ROOT=ROOT, PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, env=env, cwd=ROOT, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    assert "rccl one rank ok" in p.stdout
