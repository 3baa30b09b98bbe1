"""-m gpu, self-arming: BASELINE configs[3] over REAL RCCL ranks.

The development and grading boxes lease one MI355X, where everything multi-rank runs over gloo (two ranks sharing the
device) or on an RCCL group of one (tests/test_gpu_round2.py).  These tests skip there -- and run by themselves the day
`pytest -m gpu` sees a node with >= 2 (>= 8) devices: bench.py under torch.distributed.run with the nccl backend on the
full config-3 field, every rank's gathered catalog compared bit for bit with the single-rank sweep, and one layer of
multi-rank joint inference (parallel.DeviceJointInfer: all_gather_into_tensor on device blocks) against the one-rank
table.  The first multi-GPU lease is then evidence, not a debugging session."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _n_devices():
    try:
        import torch
        return torch.cuda.device_count()
    except Exception:
        return 0


def _launch(nproc, script_args, timeout=1200):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    port = 29300 + os.getpid() % 200
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nproc),
           "--master-addr", "127.0.0.1", "--master-port", str(port)] + script_args
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    return out.stdout


def _rccl_bench_equals_single_rank(tmp_path, n):
    import celeste_jl_amd as cel
    sys.path.insert(0, ROOT)
    import bench
    # the plain form, exactly what the driver types for N = 1: bench.py starts its N ranks itself
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(n), "--backend", "nccl", "--steps", "5",
                          "--warmup", "2", "--full", "--no-extras", "--check-dir", str(tmp_path)], capture_output=True, text=True,
                         timeout=1200, env=env)
    assert res.returncode == 0, res.stderr[-3000:]
    d = json.loads([ln for ln in res.stdout.splitlines() if ln.strip().startswith("{")][0])
    # ... and under the launcher, the way the driver starts N > 1: the same line
    out = _launch(n, [os.path.join(ROOT, "bench.py"), "--gpus", str(n), "--backend", "nccl", "--steps", "5", "--warmup", "2",
                      "--no-extras"])
    d2 = json.loads([ln for ln in out.splitlines() if ln.strip().startswith("{")][0])
    assert d2["n_gpus"] == n == d2["ranks_seen"] and d2["config"]["shard_sizes"] == d["config"]["shard_sizes"]
    S = 2000
    assert d["ranks_seen"] == n and len(d["config"]["sweep_ms_without_gather_per_rank"]) == n
    assert d["n_gpus"] == n and d["scaling"] == "strong" and d["config"]["gather_backend"] == "nccl"
    sizes = d["config"]["shard_sizes"]
    assert len(sizes) == n and sum(sizes) == S == d["config"]["sources_per_step"] and min(sizes) > 0
    assert d["config"]["catalog_gather_bytes_per_step"] == n * max(sizes) * 45 * 8
    pv = d["config"]["shard_pixel_visits"]
    assert max(pv) - min(pv) <= 0.1 * max(pv), "cost-balanced shards"
    fld = bench.build_field(2048, 1489, S, 3)
    ctx = cel.FieldContext(fld.images, fld.patches, fld.neighbors)
    v, dd, h, cnt, st = ctx.eval_batch(fld.vp, np.arange(S), 7)
    assert (st == 0).all()
    seen = np.zeros(S, dtype=bool)
    for r in range(n):
        z = np.load(os.path.join(str(tmp_path), "rank%d.npz" % r))
        assert np.array_equal(z["v"], v) and np.array_equal(z["d"], dd), "rank %d: gathered catalog != single-rank sweep" % r
        assert np.array_equal(z["h"], h[z["mine"]]), "Hessians stay with the owner"
        seen[z["mine"]] = True
    assert seen.all()
    print("%d RCCL ranks: %.0f sources/s, %.3f ms per sweep; every rank holds the single-rank catalog bit for bit"
          % (n, d["value"], d["ms_per_step"]))


@pytest.mark.skipif(_n_devices() < 2, reason="needs >= 2 GPUs (RCCL refuses two ranks on one device)")
def test_rccl_two_ranks_full_field_equals_single_rank(tmp_path):
    _rccl_bench_equals_single_rank(tmp_path, 2)


@pytest.mark.skipif(_n_devices() < 8, reason="needs 8 GPUs")
def test_rccl_eight_ranks_full_field_equals_single_rank(tmp_path):
    _rccl_bench_equals_single_rank(tmp_path, 8)


JOINT_WORKER = r'''
import os, sys
sys.path.insert(0, %(root)r)
import numpy as np, torch, torch.distributed as dist
import celeste_jl_amd as cel
from celeste_jl_amd import synthetic
from celeste_jl_amd.infer import one_node_joint_infer
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
torch.cuda.set_device(int(os.environ["LOCAL_RANK"]))
dist.init_process_group("nccl", rank=rank, world_size=world)
f = synthetic.make_field(300, 320, 60, seed=29, margin=30)
ctx = cel.FieldContext(f.images, f.patches, f.neighbors, device=int(os.environ["LOCAL_RANK"]))
tg = list(range(60))
from celeste_jl_amd.partition import estimate_time
costs = [float(estimate_time(row)) for row in f.patches]
vs = one_node_joint_infer(ctx, f.catalog, tg, f.neighbors, cel.ElboConfig(max_iters=5), batch_size=20, n_iters=1,
                          rank=rank, world=world, costs=costs)
np.save(os.path.join(%(out)r, "joint_rank%%d.npy" %% rank), vs)
dist.barrier(); dist.destroy_process_group()
'''


@pytest.mark.skipif(_n_devices() < 2, reason="needs >= 2 GPUs")
def test_rccl_joint_inference_two_ranks_equals_one_rank(tmp_path):
    """one_node_joint_infer with world = 2 over RCCL (every layer sharded, the optimised rows all-gathered on the device)
    leaves every rank with the one-rank table"""
    import celeste_jl_amd as cel
    from celeste_jl_amd import synthetic
    from celeste_jl_amd.infer import one_node_joint_infer
    script = os.path.join(str(tmp_path), "joint_worker.py")
    with open(script, "w") as fh:
        fh.write(JOINT_WORKER % {"root": ROOT, "out": str(tmp_path)})
    _launch(2, [script])
    f = synthetic.make_field(300, 320, 60, seed=29, margin=30)
    ctx = cel.FieldContext(f.images, f.patches, f.neighbors)
    ref = one_node_joint_infer(ctx, f.catalog, list(range(60)), f.neighbors, cel.ElboConfig(max_iters=5), batch_size=20, n_iters=1)
    for r in range(2):
        got = np.load(os.path.join(str(tmp_path), "joint_rank%d.npy" % r))
        assert np.array_equal(got, ref), "rank %d: max |diff| %.3e" % (r, np.abs(got - ref).max())
