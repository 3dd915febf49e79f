"""singlegpu.py / multigpu.py / bench.py end to end on the MI355X (SURVEY §4 'Integration')."""
import json
import os
import re
import subprocess
import sys

import pytest
import torch

from tests._dist_util import free_port

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, cwd, extra_env=None, timeout=600):
    env = dict(os.environ, PYTHONPATH=ROOT)
    if extra_env:
        env.update(extra_env)
    for attempt in range(3):
        r = subprocess.run([sys.executable, *args], cwd=cwd, env=env, stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, text=True, timeout=timeout)
        # free_port() cannot reserve the port it returns: another process may bind it before the child's
        # TCPStore does.  Only that host-side race is retried (nothing GPU-side failed: rendezvous precedes it)
        if r.returncode != 0 and "EADDRINUSE" in r.stdout and "MASTER_PORT" in env:
            env["MASTER_PORT"] = str(free_port())
            continue
        break
    assert r.returncode == 0, r.stdout[-4000:]
    return r.stdout


def test_singlegpu_mlp_graph_on_gpu(gpu, tmp_path):
    out = _run([os.path.join(ROOT, "singlegpu.py"), "2", "1", "--model", "mlp", "--data", "synthetic",
                "--train_size", "4096", "--test_size", "1024", "--graph", "--seed", "0", "--lr", "0.05",
                "--full_checkpoint", "--metrics", "m.jsonl"], tmp_path)
    assert "[GPU0] Epoch 1 | Batchsize: 512 | Steps: 8" in out
    acc = float(re.search(r"accuracy=(\d+\.\d\d)%", out).group(1))
    assert acc > 15.0, out
    sd = torch.load(tmp_path / "checkpoint.pt", weights_only=True)
    assert sd["fc0.weight"].dtype == torch.float32 and sd["fc0.weight"].shape == (4096, 3072)
    recs = [json.loads(ln) for ln in open(tmp_path / "m.jsonl")]
    assert any("samples_per_s" in r for r in recs)


def test_singlegpu_vgg_native_on_gpu(gpu, tmp_path):
    out = _run([os.path.join(ROOT, "singlegpu.py"), "1", "1", "--data", "synthetic", "--train_size", "2048",
                "--test_size", "512", "--dtype", "bf16"], tmp_path)
    assert "fp32 model has size=35.20 MiB" in out
    assert re.search(r"fp32 model has accuracy=\d+\.\d\d%", out)


def test_singlegpu_reference_command_trains_fp32(gpu, tmp_path):
    """``python singlegpu.py E S`` with no flags: the reference's VGG at the reference's precision (fp32)."""
    out = _run([os.path.join(ROOT, "singlegpu.py"), "1", "1", "--data", "synthetic", "--train_size", "1024",
                "--test_size", "512", "--metrics", "m.jsonl"], tmp_path)
    assert "[GPU0] Epoch 0 | Batchsize: 512 | Steps: 2" in out
    assert "fp32 model has size=35.20 MiB" in out
    sd = torch.load(tmp_path / "checkpoint.pt", weights_only=True)
    assert all(v.dtype in (torch.float32, torch.int64) for v in sd.values())


def test_multigpu_single_rank_rccl_sharded(gpu, tmp_path):
    """The distributed entry point with the native RCCL communicator at world size 1 (ZeRO-1, bf16 grads)."""
    out = _run([os.path.join(ROOT, "multigpu.py"), "1", "1", "--nprocs", "1", "--model", "mlp", "--data",
                "synthetic", "--train_size", "2048", "--test_size", "512", "--shard_optimizer", "--grad_dtype",
                "bf16", "--overlap_optimizer", "--metrics", "m.jsonl", "--dtype", "bf16"], tmp_path,
               extra_env={"MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(free_port())})
    assert "[GPU0] Epoch 0 | Batchsize: 512 | Steps: 4" in out
    recs = [json.loads(ln) for ln in open(tmp_path / "m.jsonl")]
    assert any("loss_mean_ranks" in r for r in recs)  # all-reduced over the (single-rank) group


@pytest.mark.parametrize("shard", [0, 1])
def test_bench_ddp_single_comm_stats(gpu, tmp_path, shard):
    """bench.py --ddp_single: the RCCL reducer at world size 1 reports per-step comm / exposed time
    (replicated optimizer by default, ZeRO-1 when asked)."""
    out = _run([os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "10", "--warmup", "3", "--ddp_single",
                "--shard_optimizer", str(shard)],
               tmp_path, extra_env={"MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(free_port()),
                                    "DDPX_COMM_SKIP_IDENTITY": "0"})  # real RCCL calls at world size 1
    rec = json.loads([ln for ln in out.splitlines() if ln.startswith("{")][0])
    assert rec["config"]["ddp"] and rec["config"]["replicas_consistent"]
    assert rec["config"]["sharded_optimizer"] is bool(shard)
    assert rec["config"]["comm_ms_per_step"] > 0


def test_bench_n_gt_1_paths_at_world_size_1(gpu, tmp_path):
    """Every bench.py branch that otherwise runs only at N > 1, executed on the GPU before the driver's 8-GPU
    job does: the start-up calibration on the real RcclComm (replicated AND ZeRO-1
    candidates, RCCL identity collectives really issued, each candidate graph-captured), the stock baseline
    wrapped in torch DDP over its own ``dist.new_group(backend="nccl")``, and the replica digest exchange."""
    out = _run([os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "10", "--warmup", "3", "--ddp_single",
                "--stock_ddp", "1", "--stock_steps", "5", "--train_size", "8192", "--full"],
               tmp_path, extra_env={"MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(free_port()),
                                    "DDPX_COMM_SKIP_IDENTITY": "0"})
    rec = json.loads([ln for ln in out.splitlines() if ln.startswith("{")][0])
    c = rec["config"]
    assert c["bucket_plan"] == "calibrated", c
    table = c["calibration"]["step_ms"]
    assert any(k.startswith("zero1") for k in table) and any(k.startswith("allreduce") for k in table), table
    assert all(v > 0 for v in table.values()) and c["calibration"]["chosen"] in table
    assert c["graph"] is True and c["graph_error"] is None
    # the DDP job's placement: the stock torch-DDP run starts only after the ddpx line is out
    assert c["stock_same_run"]["placement"].startswith("after this line")
    assert out.index('{"metric"') < out.index("STOCK {")
    tail = json.loads(out.split("STOCK ", 1)[1].splitlines()[0])
    assert "torch DDP" in tail["stock_same_run"]["recipe"] and tail["vs_stock_same_run"] > 0, tail
    assert c["replicas_consistent"] is True and c["ddp"] is True


def test_bench_ddp_job_survives_optional_failures(gpu, tmp_path):
    """VERDICT r5 item 1 on the GPU (the N > 1 layout at world size 1): a failure injected into the stock
    torch-DDP run (after its NCCL group and DDP model exist) and into every ZeRO-1 calibration trial (first
    training step, real RcclComm, graph capture) — rc 0, the ddpx line, the ZeRO-1 candidates dropped, the stock
    error agreed and reported."""
    out = _run([os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "10", "--warmup", "3", "--ddp_single",
                "--stock_ddp", "1", "--stock_steps", "5", "--train_size", "8192", "--full"],
               tmp_path, extra_env={"MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(free_port()),
                                    "DDPX_COMM_SKIP_IDENTITY": "0", "DDPX_BENCH_INJECT": "calib:zero1,stock_run"})
    lines = [ln for ln in out.splitlines() if ln.startswith('{"metric"')]
    assert len(lines) == 1, out[-3000:]
    c = json.loads(lines[0])["config"]
    cal = c["calibration"]
    assert cal["dropped"] and all(k.startswith("zero1") for k in cal["dropped"]), cal
    assert cal["chosen"].startswith("allreduce") and c["sharded_optimizer"] is False
    assert all(isinstance(v, dict) == k.startswith("zero1") for k, v in cal["step_ms"].items()), cal
    assert c["graph"] is True and c["replicas_consistent"] is True
    tail = json.loads(out.split("STOCK ", 1)[1].splitlines()[0])
    assert "InjectedFault" in tail["stock_same_run"]["error"] and tail["vs_stock_same_run"] is None


def test_bench_sim_world_builds_the_n_rank_layout(gpu, tmp_path):
    """``--ddp_single --sim_world 4 --shard_optimizer 1``: the 4-rank ZeRO-1 layout (1/4 shards, shadow gathers) on a
    one-rank communicator with every collective skipped — the per-rank compute table of docs/SCALING.md."""
    out = _run([os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "10", "--warmup", "3", "--ddp_single",
                "--sim_world", "4", "--shard_optimizer", "1", "--bucket_plan", "default", "--stock_ref", "0"],
               tmp_path, extra_env={"MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(free_port())})
    rec = json.loads([ln for ln in out.splitlines() if ln.startswith('{"metric"')][0])
    c = rec["config"]
    assert c["sim_world"] == 4 and c["sharded_optimizer"] is True and c["graph"] is True
    assert rec["n_gpus"] == 1 and rec["value"] > 0


def test_bench_contract_one_gpu(gpu, tmp_path):
    out = _run([os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "10", "--warmup", "3"], tmp_path)
    lines = [ln for ln in out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    rec = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config"):
        assert k in rec
    assert rec["n_gpus"] == 1 and rec["steps"] == 10 and rec["value"] > 0 and rec["dtype"] == "bf16"


@pytest.mark.parametrize("model", ["mlp", "vgg"])
def test_bench_batch_prefetch_trains_identically(gpu, tmp_path, model):
    """The double-buffered batch prefetch (augment of step k+1 on a side stream during step k) trains on the
    same batches in the same order: final loss and fp32 master + momentum bytes equal the in-step augment's,
    over an odd number of graph replays (both buffer parities, eager warm-up steps included)."""
    recs = []
    for pf in (1, 0):
        out = _run([os.path.join(ROOT, "bench.py"), "--gpus", "1", "--model", model, "--steps", "7", "--warmup", "4",
                    "--stock_ref", "0", "--digest", "1", "--prefetch_batch", str(pf)], tmp_path)
        recs.append(json.loads([ln for ln in out.splitlines() if ln.startswith("{")][-1]))
    a, b = recs
    assert a["config"]["prefetch_batch"] is True and b["config"]["prefetch_batch"] is False
    assert a["config"]["graph"] and b["config"]["graph"]
    assert a["config"]["final_loss"] == b["config"]["final_loss"]
    assert a["config"]["master_digest"] == b["config"]["master_digest"] is not None


def test_multigpu_reference_command_fp32_native_calibrated(gpu, tmp_path):
    """``python multigpu.py E S`` with the reference's defaults (VGG, fp32, batch 512) on the GPU, one rank: the
    native fp32 kernels under DDP over the native RCCL communicator, with the bucket plan calibrated by training
    steps, HIP graphs and per-bucket optimizer overlap — the tuned path behind the reference's own entry point."""
    out = _run([os.path.join(ROOT, "multigpu.py"), "1", "1", "--nprocs", "1", "--data", "synthetic", "--train_size",
                "2048", "--test_size", "512"], tmp_path,
               extra_env={"MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(free_port())})
    assert "[GPU0] Epoch 0 | Batchsize: 512 | Steps: 4" in out
    assert "fp32 model has size=35.20 MiB" in out
    assert "bucket plan: calibrated" in out, out
    sd = torch.load(tmp_path / "checkpoint.pt", weights_only=True)
    assert all(v.dtype in (torch.float32, torch.int64) for v in sd.values())


def test_multigpu_reference_launch_without_nprocs(gpu, tmp_path):
    """``python multigpu.py E S`` exactly as the reference launches it (no --nprocs: world size = the node's GPU
    count, /root/reference/multigpu.py:262-263), counted without initialising HIP in the launcher
    (ddpx.utils.devices), which then mp.spawns the ranks."""
    from ddpx.utils.devices import visible_gpu_count
    n = visible_gpu_count()
    assert n == torch.cuda.device_count(), (n, torch.cuda.device_count())
    if n != 1:
        pytest.skip("the one-rank launch check needs a one-GPU box")
    out = _run([os.path.join(ROOT, "multigpu.py"), "1", "1", "--data", "synthetic", "--train_size", "2048",
                "--test_size", "512"], tmp_path, extra_env={"MASTER_ADDR": "127.0.0.1",
                                                              "MASTER_PORT": str(free_port())})
    assert "[GPU0] Epoch 0 | Batchsize: 512 | Steps: 4" in out
    assert "fp32 model has accuracy=" in out
    assert "[GPU1]" not in out
