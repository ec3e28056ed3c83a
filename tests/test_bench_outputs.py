"""bench.py's plain run, --full and --dump-outputs: a plain run times the steps
and prints the line, --full adds the side measurements, and --dump-outputs
writes what the last timed step returned, the same problems on every run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIDE_KEYS = ("ingest", "explicit_inverse", "rank_update_plugin", "cpu_baseline_structured", "cpu_baseline_allcores")


def _env(**extra):
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "LOCAL_WORLD_SIZE")}
    env.update(extra)
    return env


def _bench(args, env):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True,
                       timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_dump_outputs_whole_batch_and_seeded_sample(tmp_path, monkeypatch):
    """Every per-problem array lands as float64 [rows, width]; under the byte
    budget all B problems are rows, above it the rows are one sorted sample of
    problem indices shared by every array, the same on every call."""
    import torch
    import bench
    B, n, k = 37, 5, 7
    out = dict(x=torch.arange(B * n, dtype=torch.float64), z=torch.arange(B * k, dtype=torch.float64) + 0.5,
               iters=torch.arange(B, dtype=torch.int32), y=torch.empty(1, dtype=torch.float64))
    bench.dump_outputs(str(tmp_path / "all"), out, B, skip=("y",))
    assert sorted(os.listdir(tmp_path / "all")) == ["iters.npy", "x.npy", "z.npy"]
    x = np.load(tmp_path / "all" / "x.npy")
    assert x.dtype == np.float64 and x.shape == (B, n) and (x.ravel() == np.arange(B * n)).all()
    it = np.load(tmp_path / "all" / "iters.npy")
    assert it.dtype == np.float64 and it.shape == (B, 1)
    # room for 10 problems of n + k + 1 doubles
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 10 * 8 * (n + k + 1) + 7)
    for d in ("s1", "s2"):
        bench.dump_outputs(str(tmp_path / d), out, B, skip=("y",))
    idx = np.load(tmp_path / "s1" / "sample_index.npy")
    assert idx.dtype == np.float64 and idx.shape == (10,)
    assert (np.diff(idx) > 0).all() and 0 <= idx[0] and idx[-1] < B
    x, z, it = (np.load(tmp_path / "s1" / f) for f in ("x.npy", "z.npy", "iters.npy"))
    assert (it[:, 0] == idx).all() and (x[:, 0] == idx * n).all() and (z[:, 0] == idx * k + 0.5).all()
    assert sum(os.path.getsize(tmp_path / "s1" / f) for f in ("x.npy", "z.npy", "iters.npy")) <= 10 * 8 * (n + k + 1) + 3 * 128
    for f in os.listdir(tmp_path / "s1"):
        assert (np.load(tmp_path / "s1" / f) == np.load(tmp_path / "s2" / f)).all(), f


def test_bench_stub_run_dumps_last_step(tmp_path):
    """`--dump-outputs DIR` on the stub solve (CPU only): the outcome arrays of
    the last timed step, float64, one row per problem; `--steps` is the number
    of timed steps the line accounts for."""
    B, K, steps = 32, 8, 3
    line = _bench(["--steps", str(steps), "--warmup", "1", "--batch", str(B), "--stub-solve",
                   "--dump-outputs", str(tmp_path / "d")], _env(CUDA_VISIBLE_DEVICES="", OMP_NUM_THREADS="1"))
    assert line["steps"] == steps
    assert abs(line["value"] * line["ms_per_step"] * steps / 1e3 - B * K * steps) <= 1e-6 * B * K * steps
    assert sorted(os.listdir(tmp_path / "d")) == ["iters.npy", "res.npy", "status.npy"]
    it = np.load(tmp_path / "d" / "iters.npy")
    assert it.dtype == np.float64 and it.shape == (B, 1) and (it == K).all()
    assert np.load(tmp_path / "d" / "res.npy").shape == (B, 3)


@pytest.mark.gpu
def test_bench_plain_run_is_lean_and_dumps_the_solve(tmp_path):
    """A plain run carries no side measurement (no ingest / other-mode / CPU
    lines), and its dump is bit for bit what batch_solve returns for the same
    generated problems (C2 shape, a batch that is no multiple of the block)."""
    import torch
    import socp_amd as S
    from socp_amd.configs import C2 as cfg
    B, steps = 301, 2
    line = _bench(["--gpus", "1", "--steps", str(steps), "--warmup", "1", "--batch", str(B),
                   "--dump-outputs", str(tmp_path / "d")], _env())
    assert line["steps"] == steps and line["ms_per_step"] > 0 and line["dtype"] == "f64"
    assert line["unit"] == "problem-iterations/s" and line["higher_is_better"] is True
    assert line["cpu_baseline"] is None
    assert not [key for key in SIDE_KEYS if key in line]
    n, m, k = cfg.n, cfg.m, cfg.k
    c, A, b, G, h = S.generate(cfg.cones, B, n, m, k, cfg.seed)
    sing = torch.zeros(B, dtype=torch.uint8, device=G.device)
    ref = S.batch_solve(cfg.cones, n, m, k, c, A, b, G, h, sing, maxit=cfg.fixed_k, tol=0.0)
    S.default_context().sync()
    done = int(ref["iters"].sum().item()) * steps  # value = executed problem-iterations / the timed steps' time
    assert abs(line["value"] * line["ms_per_step"] * steps / 1e3 - done) <= 1e-6 * done
    assert sorted(os.listdir(tmp_path / "d")) == sorted(key + ".npy" for key in ref)
    for key, w in (("x", n), ("y", m), ("z", k), ("s", k), ("iters", 1), ("status", 1)):
        got = np.load(tmp_path / "d" / (key + ".npy"))
        assert got.dtype == np.float64 and got.shape == (B, w), key
        assert np.array_equal(got, ref[key].cpu().numpy().astype(np.float64).reshape(B, w), equal_nan=True), key


@pytest.mark.gpu
def test_bench_full_adds_the_side_measurements():
    """`--full` (here without the CPU leg): the same headline block plus the
    PCIe-inclusive ingest line and the explicit-inverse and rank-update
    summaries, each a positive rate."""
    line = _bench(["--gpus", "1", "--steps", "1", "--warmup", "1", "--batch", "301", "--full", "--no-cpu"], _env())
    assert line["steps"] == 1 and line["ms_per_step"] > 0 and line["cpu_baseline"] is None
    assert line["ingest"]["value"] > 0 and line["ingest"]["pageable"]["value"] > 0
    assert line["explicit_inverse"]["value_kernel"] > 0
    assert line["rank_update_plugin"]["value"] > 0 and line["rank_update_plugin"]["solve_socp"]["value"] > 0
