"""Driver-contract test for bench.py: one JSON line on stdout with the
exact fields and semantics the round driver parses (BASELINE.json metric,
whole-job aggregate value, ms_per_step consistency)."""

import json
import os
import subprocess
import sys

import pytest


REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = ["--steps", "2", "--warmup", "0", "--model", "tiny-llama", "--batch", "2",
        "--max-new", "8", "--prompt-len", "64"]


def _cpu_env():
    """These are the CPU (fp32 / gloo) contract runs: the tiny test model's
    head_dim is not one the HIP attention kernels take, so hide any GPU from
    the bench subprocess instead of failing where one is present."""
    env = dict(os.environ)
    env["HIP_VISIBLE_DEVICES"] = ""
    env["CUDA_VISIBLE_DEVICES"] = ""
    return env


def _run_bench(extra):
    out = subprocess.run(
        [sys.executable, "bench.py", *TINY, *extra],
        cwd=REPO, capture_output=True, text=True, timeout=500, env=_cpu_env(),
    )
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.strip().splitlines() if l.strip()]
    assert len(lines) == 1, f"exactly ONE json line expected, got {len(lines)}"
    return json.loads(lines[0])


@pytest.fixture(scope="module")
def plain_run(tmp_path_factory):
    """ONE plain run (shared): its result line and its --dump-outputs dir."""
    dump = tmp_path_factory.mktemp("bench_plain")
    return _run_bench(["--dump-outputs", str(dump)]), dump


@pytest.mark.timeout(600)
def test_bench_json_contract(plain_run):
    d, _ = plain_run

    assert d["metric"] == "end_to_end_consensus_requests_per_s"
    assert d["unit"] == "req/s"
    assert d["higher_is_better"] is True
    assert d["scaling"] in ("weak", "strong")
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 0
    assert d["value"] > 0
    assert d["vs_baseline"] == pytest.approx(d["value"] / 1.2, rel=1e-3)
    # value is the WHOLE-JOB rate; ms_per_step must be consistent with it
    assert d["ms_per_step"] == pytest.approx(
        1000.0 * d["config"]["global_batch"] / d["value"], rel=1e-2)
    assert d["dtype"] in ("bf16", "float32")
    assert "synthetic" in d["data"]
    cfg = d["config"]
    for k in ("model", "n", "global_batch", "seq_len", "parallelism",
              "completions_per_s", "consensus_latency_s_per_request",
              "batch_wall_s"):
        assert k in cfg, k
    assert cfg["parallelism"] == "dp1 tp1"


@pytest.mark.timeout(600)
def test_bench_dump_outputs_and_full(plain_run, tmp_path):
    """--dump-outputs writes the last timed step's responses as float .npy
    arrays, one row per request; the inputs depend only on the arguments, so
    a second run (here with --full, which must leave the headline run as it
    is) sees the same prompts and returns the same responses."""
    import numpy as np

    d, dump = plain_run
    names = sorted(os.listdir(dump))
    assert names == ["content.npy", "content_len.npy", "likelihoods.npy", "usage.npy"]
    arrs = {n: np.load(os.path.join(dump, n)) for n in names}
    assert all(a.dtype in (np.float32, np.float64) for a in arrs.values())
    assert sum(a.nbytes for a in arrs.values()) <= 64 * 2**20
    batch, n = d["config"]["global_batch"], d["config"]["n"]
    assert arrs["content.npy"].shape[:2] == (batch, n + 1)     # consensus + n originals
    assert arrs["content_len.npy"].shape == (batch, n + 1)
    assert (arrs["content_len.npy"] >= 0).all()
    assert arrs["usage.npy"].shape == (batch, 3)
    assert (arrs["usage.npy"][:, 0] + arrs["usage.npy"][:, 1] == arrs["usage.npy"][:, 2]).all()
    lik = arrs["likelihoods.npy"]
    assert lik.shape[0] == batch and ((lik >= 0) & (lik <= 1) | (lik == -1)).all()

    d2 = _run_bench(["--full", "--dump-outputs", str(tmp_path)])
    assert set(d2) == set(d) and set(d2["config"]) == set(d["config"])
    assert d2["steps"] == 2 and d2["metric"] == d["metric"]
    again = {n: np.load(os.path.join(tmp_path, n)) for n in names}
    for name in names:
        np.testing.assert_array_equal(again[name], arrs[name], err_msg=name)


@pytest.mark.timeout(600)
def test_bench_driver_multiproc_invocation(tmp_path):
    """The EXACT shape the driver uses for SCALE_rNN: torch.distributed.run
    with N ranks — on CPU this exercises the gloo/dp path end to end and
    must still print exactly ONE JSON line (rank 0) with the whole-job
    aggregate value."""
    env = _cpu_env()
    env["MASTER_ADDR"] = "127.0.0.1"
    out = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
         "--master-port", "29841", "bench.py", "--gpus", "2",
         "--steps", "2", "--warmup", "0", "--model", "tiny-llama",
         "--batch", "2", "--max-new", "6", "--prompt-len", "48"],
        cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
        capture_output=True, text=True, timeout=500, env=env,
    )
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.strip().splitlines()
             if l.strip().startswith("{")]
    assert len(lines) == 1, f"exactly ONE json line expected: {out.stdout[-800:]}"
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2
    assert d["scaling"] == "weak"
    assert d["config"]["parallelism"].startswith("dp2")
    # whole-job aggregate: 2 ranks x per-rank batch
    assert d["config"]["global_batch"] == 4
    assert d["value"] > 0


@pytest.mark.timeout(600)
def test_bench_tp_serving_invocation(tmp_path):
    """bench.py --parallel tp: rank 0 drives the scheduler, rank 1 replays
    (TPCoordinator/TPFollower) — the full TP serving stack under the bench
    entry, on CPU/gloo."""
    env = _cpu_env()
    env["MASTER_ADDR"] = "127.0.0.1"
    out = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
         "--master-port", "29843", "bench.py", "--gpus", "2",
         "--parallel", "tp", "--steps", "2", "--warmup", "0",
         "--model", "tiny-llama", "--batch", "2", "--max-new", "6",
         "--prompt-len", "48"],
        cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
        capture_output=True, text=True, timeout=500, env=env,
    )
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.strip().splitlines()
             if l.strip().startswith("{")]
    assert len(lines) == 1, f"exactly ONE json line expected: {out.stdout[-800:]}"
    d = json.loads(lines[0])
    assert d["config"]["parallelism"] == "tp2"
    assert d["value"] > 0
