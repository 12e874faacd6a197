"""CPU (gloo, world_size 2): bench.py's own multi-rank code path — self-spawned ranks, clip teams (frame-parallel encode, point-to-point
token exchange, sequence-parallel prefill), max-over-ranks timing, the JSON contract — at reduced depth on the contract backend (`--dry-cpu`).
A plumbing check: the numbers mean nothing, the structure of the line and the absence of a launcher requirement do."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--dry-cpu", "--steps", "1", "--warmup", "0", "--vit-depth", "1", "--qformer-layers", "2", "--llm-layers", "1", "--frames", "2"]


def _run(extra, timeout=900, threads=None):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    if threads:   # many ranks on few cores: one BLAS thread per rank (8 ranks x 8 threads on 8 vCPUs spend their time in the scheduler)
        env.update(OMP_NUM_THREADS=str(threads), MKL_NUM_THREADS=str(threads))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + SMALL + extra, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-2000:] + "\n" + r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.mark.parametrize("config,scaling,batch", [("c3", "strong", 4), ("c2", "weak", 2)])
def test_bench_self_spawns_two_ranks(config, scaling, batch):
    res = _run(["--gpus", "2", "--config", config, "--fp-clips", "1", "--full"])
    assert res["n_gpus"] == 2 and res["scaling"] == scaling and res["config"]["name"] == config
    assert res["config"]["global_batch"] == batch and res["steps"] == 1 and res["higher_is_better"] is True
    assert res["value"] > 0 and res["ms_per_step"] > 0
    assert "clip teams over 2 ranks" in res["config"]["parallelism"] and "DRY RUN" in res["data"]
    assert res["loss"] == res["loss"], "rank 0 owns clip 0: its loss must be a number"
    assert res["token_exchange_in_step"] is False    # 2 ranks, 4 (c3) or 2 (c2) clips: whole clips per rank, teams of one
    assert res["frames_per_rank"] == [batch, batch] and res["rccl_ranks"] == 2
    if config == "c3":
        assert res["config"]["video_tokens_per_clip"] == 2 * 32 and "residual" in res["config"]["workload"]   # R clamped to the 2 frames of the dry run
        assert res["plan"]["teams"] == [[0], [1], [0], [1]]
        assert "frame_parallel" not in res            # the c3 line IS the frame-parallel experiment
    else:
        # `bench.py --gpus N --full` (no --config) must carry the north star's experiment: c3 strong scaling, rank 0 alone first, then all
        # ranks as clip teams (here --fp-clips 1: ONE clip on 2 ranks = a team of two, 1 frame each, point-to-point exchange, sequence-parallel
        # prefill), the received blocks checked against the single-GPU encode, throughput AND one-batch latency timed
        fp = res["frame_parallel"]
        assert fp["config"] == "c3" and fp["scaling"] == "strong" and fp["token_exchange_in_step"] is True and fp["sequence_parallel_prefill"] is True
        assert fp["ms_per_step_1gpu"] > 0 and fp["ms_per_step"] > 0 and abs(fp["speedup"] - fp["ms_per_step_1gpu"] / fp["ms_per_step"]) < 1e-2
        assert fp["latency_ms"] > 0 and abs(fp["latency_speedup"] - fp["ms_per_step_1gpu"] / fp["latency_ms"]) < 1e-2
        assert fp["plan"]["teams"] == [[0, 1]] and fp["plan"]["frames"] == [[[0, 1], [1, 2]]]
        assert fp["frames_per_rank"] == [1, 1] and fp["clips_per_rank"] == [1, 1] and fp["token_exchange_us"] > 0
        assert fp["received_blocks_bit_identical"] is True and fp["received_blocks_max_abs_diff"] == 0.0
        assert fp["token_exchange_bytes_sent_per_rank"] == [32 * 4096 * 4] * 2
        oo = fp["owner_only_throughput_plan"]     # the same batch with the owner prefilling alone (helpers return before pooling): timed next to the default
        assert oo["ms_per_step"] > 0 and oo["latency_ms"] > 0 and oo["clips_per_rank"] == [1, 0] and sum(oo["frames_per_rank"]) == 2


def test_bench_self_spawns_eight_ranks_clip_teams_of_two():
    """VERDICT r05 #8c: the N = 8 plan of `bench.py --gpus 8 --full` — c3's 4 clips as 4 teams of 2 ranks, point-to-point token exchange,
    sequence-parallel prefill inside every team, the loss run along the team — executed end to end by 8 gloo processes (contract backend, reduced depth:
    plumbing, not a measurement; no byte has crossed RCCL for this repository yet)."""
    res = _run(["--gpus", "8", "--config", "c2", "--full"], timeout=1500, threads=1)
    assert res["n_gpus"] == 8 and res["rccl_ranks"] == 8 and res["config"]["global_batch"] == 8 and res["value"] > 0
    assert res["plan"]["teams"] == [[r] for r in range(8)] and res["token_exchange_in_step"] is False     # c2 weak scaling: one clip per rank, nothing on the wire
    fp = res["frame_parallel"]
    assert fp["config"] == "c3" and fp["scaling"] == "strong" and fp["sequence_parallel_prefill"] is True and fp["token_exchange_in_step"] is True
    assert fp["plan"]["teams"] == [[0, 4], [1, 5], [2, 6], [3, 7]] and all(fp["plan"]["sp"])
    assert fp["plan"]["frames"] == [[[0, 1], [1, 2]]] * 4 and fp["frames_per_rank"] == [1] * 8 and fp["clips_per_rank"] == [1] * 8
    assert fp["received_blocks_bit_identical"] is True and fp["received_blocks_max_abs_diff"] == 0.0
    assert fp["ms_per_step"] > 0 and fp["latency_ms"] > 0 and fp["ms_per_step_1gpu"] > 0
    oo = fp["owner_only_throughput_plan"]
    assert sum(oo["frames_per_rank"]) == 8 and sum(oo["clips_per_rank"]) == 4


def test_bench_single_rank_line_carries_projection_blocks_and_telemetry_keys():
    """N = 1, --full: the c2 line must carry the frame_parallel_projection block (c3 on one GPU, every kind of rank of the
    TeamPlan at N = 2 / 4 / 8 played alone: throughput_ms AND latency_ms from the measured shares + a modelled wire, labelled unmeasured),
    ms_per_step_blocks and the telemetry key (null without a GPU)."""
    res = _run(["--gpus", "1", "--full"])
    assert res["n_gpus"] == 1 and res["config"]["name"] == "c2" and res["steps"] == 1
    assert res["ms_per_step_blocks"]["steps"] == [1] and len(res["ms_per_step_blocks"]["ms"]) == 1 and "telemetry" in res
    pj = res["frame_parallel_projection"]
    assert pj["config"] == "c3" and pj["ms_per_step_1gpu"] > 0 and set(pj["n"]) == {"2", "4", "8", "8_owner_only", "8_owner_only_latency"} and "UNMEASURED" in pj["status"]
    for N, blk in pj["n"].items():
        N = int(N.split("_")[0])
        assert sum(sh["ranks_of_this_kind"] for sh in blk["shares"]) == N and all(sh["step_ms"] > 0 and sh["enc_ms"] > 0 for sh in blk["shares"])
        assert sum(sum(sh["frames"]) * sh["ranks_of_this_kind"] for sh in blk["shares"]) == 4 * 2        # every frame encoded exactly once
        slow = max(sh["step_ms"] for sh in blk["shares"])
        assert abs(blk["throughput_ms"] - (slow + blk["token_exchange_ms_modelled"] + blk["kv_lag_ms_modelled"])) < 2e-3
        assert blk["latency_ms"] > 0 and abs(blk["latency_speedup"] - pj["ms_per_step_1gpu"] / blk["latency_ms"]) < 2e-2
        assert abs(blk["throughput_speedup"] - pj["ms_per_step_1gpu"] / blk["throughput_ms"]) < 2e-2
        teams = blk["plan"]["teams"]
        assert (blk["token_exchange_ms_modelled"] > 0) == any(len(t) > 1 for t in teams)
    assert pj["n"]["4"]["plan"]["teams"] == [[0], [1], [2], [3]] and pj["n"]["4"]["kv_lag_ms_modelled"] == 0      # one clip per rank: nothing on the wire
    assert pj["n"]["8"]["plan"]["teams"] == [[0, 4], [1, 5], [2, 6], [3, 7]] and all(pj["n"]["8"]["plan"]["sp"])
    assert any(p["sequence_parallel"] for sh in pj["n"]["8"]["shares"] for p in sh["prefill"])
    chk = pj["sequence_parallel_check"]      # the two members of clip 0's team at N = 8, played on this process: their rows tile the sequence and equal the 1-process logits
    blk = next(v for k, v in chk.items() if isinstance(v, dict))     # one block per numerics mode checked (the dry run: its fp32 contract backend only)
    rows, dif = blk["rows"], blk["logits_max_abs_diff_vs_1gpu"]
    assert chk["ranks"] == [0, 4] and rows[0][0] == 0 and rows[0][1] == rows[1][0] and max(dif) <= 1e-3
    oo = pj["n"]["8_owner_only"]      # the owner prefills alone and encodes fewer frames: helpers have no prefill share
    assert not any(oo["plan"]["sp"]) and sorted(len(sh["prefill"]) for sh in oo["shares"]) == [0, 1] and oo["kv_lag_ms_modelled"] == 0


def test_bench_watchdog_keeps_the_headline_when_the_frame_parallel_block_stalls():
    """the c3 block (--full) has never run on a multi-GPU node: if it does not finish in --fp-timeout seconds, rank 0 still prints the (complete) headline line,
    with the reason in place of the block, and every rank exits 0"""
    res = _run(["--gpus", "2", "--fp-clips", "1", "--fp-timeout", "0.5", "--full"])
    assert res["n_gpus"] == 2 and res["value"] > 0 and res["ms_per_step"] > 0
    assert "watchdog" in res["frame_parallel"]["error"]


@pytest.mark.parametrize("config", ["c4", "c5"])
def test_bench_mvm_configs_dry(config):
    """--config c4 / c5 (BASELINE configs[3] / [4]): mask drawn by the package's generator from the seeded numpy stream and injected, two
    prefills per step, BT-Adapter backbone for c5."""
    res = _run(["--gpus", "1", "--config", config, "--no-extra-legs"])
    assert res["config"]["name"] == config and "MVM branch" in res["config"]["workload"] and res["loss"] == res["loss"]
    assert ("BT-Adapter" in res["config"]["workload"]) == (config == "c5")
    assert res["config"]["video_tokens_per_clip"] == 2 * 32


def test_bench_plain_run_times_the_headline_only_and_dumps_its_outputs(tmp_path):
    """without --full the line is the headline of exactly --steps timed steps: no parity, roofline, telemetry, single-stream bracket, numerics legs,
    projection or CPU baseline; --dump-outputs writes what the last timed step returned (float32 .npy)"""
    import numpy as np
    res = _run(["--gpus", "1", "--steps", "2", "--dump-outputs", str(tmp_path / "out")])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in res, k
    assert res["steps"] == 2 and res["ms_per_step_blocks"]["steps"] == [2] and res["value"] > 0 and res["ms_per_step"] > 0
    for k in ("parity", "roofline", "single_stream", "fp16", "frame_parallel_projection", "frame_parallel", "cpu_baseline"):
        assert k not in res, k
    assert res["telemetry"] is None
    loss, logits = np.load(tmp_path / "out" / "loss.npy"), np.load(tmp_path / "out" / "logits.npy")
    assert loss.dtype == np.float32 and logits.dtype == np.float32
    assert loss.shape == (1,) and abs(float(loss[0]) - res["loss"]) < 1e-4
    assert logits.shape == (res["config"]["seq_len"], 32000) and np.isfinite(logits).all()
    assert not (tmp_path / "out" / "logits_rows.npy").exists()      # small enough to be written whole


def test_dump_outputs_samples_large_logits_with_a_fixed_seed(tmp_path):
    """logits above the dump's budget: a fixed sample of their rows (the same rows every run), stored with the row numbers; the whole dump stays under 64 MB"""
    import types
    import numpy as np
    import torch
    import bench
    lg = torch.randn(1, 576, 32000)
    out = types.SimpleNamespace(loss=torch.tensor(2.5), loss_mvm=None, logits=lg)
    assert bench.dump_outputs(out, str(tmp_path / "a")) == ["logits", "logits_rows", "loss"]
    bench.dump_outputs(out, str(tmp_path / "b"))
    rows = np.load(tmp_path / "a" / "logits_rows.npy")
    assert np.array_equal(rows, np.load(tmp_path / "b" / "logits_rows.npy"))
    r = rows.astype(np.int64)
    assert (np.diff(r) > 0).all() and r[0] >= 0 and r[-1] < 576 and len(r) == bench.DUMP_LOGITS_BYTES // (32000 * 4)
    assert np.array_equal(np.load(tmp_path / "a" / "logits.npy"), lg[0, r].numpy())
    assert sum(f.stat().st_size for f in (tmp_path / "a").iterdir()) <= 64e6
    assert float(np.load(tmp_path / "a" / "loss.npy")[0]) == 2.5


def test_bench_launcher_environment_is_honoured(monkeypatch):
    """under `python -m torch.distributed.run` bench.py must NOT spawn again: WORLD_SIZE in the environment wins over --gpus"""
    import importlib
    import bench
    importlib.reload(bench)
    called = {}
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setattr(bench, "spawn_ranks", lambda a: called.setdefault("spawn", True) or 0)
    monkeypatch.setattr(bench, "run_rank", lambda a: called.setdefault("rank", a.gpus))
    monkeypatch.setattr("sys.argv", ["bench.py", "--gpus", "2"])
    bench.main()
    assert called == {"rank": 2}
    monkeypatch.delenv("WORLD_SIZE")
    called.clear()
    with pytest.raises(SystemExit):
        bench.main()
    assert called == {"spawn": True}
