"""bench.py contract at world size 1, 2 and 4 without GPUs (--device cpu: gloo + the fp32
reference model). The driver runs bench.py either under torch.distributed.run or as
`python bench.py --gpus N` (bench.py then spawns the N ranks itself); this rehearses
everything around the kernels for both: rendezvous on 127.0.0.1, C1 broadcast, C2
all-reduce, the barrier-bracketed timing, max over ranks, and exactly ONE JSON line from
rank 0 with the whole-job aggregate value."""
import json
import os
import socket
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
        "scaling", "vs_baseline", "dtype", "data", "config"}


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run(world, model, extra, torchrun=True):
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="", OMP_NUM_THREADS="1")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    args = ["bench.py", "--gpus", str(world), "--steps", "3", "--warmup", "1", "--device", "cpu",
            "--model", model] + extra
    if world > 1 and torchrun:
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}",
               "--master-addr", "127.0.0.1", "--master-port", str(_port())] + args
    else:
        cmd = [sys.executable] + args
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, cwd=ROOT, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.mark.parametrize("world", [1, 2, 4])
def test_bench_json_contract_lstm(world):
    B = 4
    rec = _run(world, "lstm", ["--batch", str(B), "--seq", "6", "--hidden", "16"])
    assert KEYS <= set(rec)
    assert rec["n_gpus"] == world and rec["steps"] == 3 and rec["warmup"] == 1
    assert rec["config"]["global_batch"] == B * world and rec["config"]["parallelism"] == f"dp{world}"
    assert rec["config"]["seq_len"] == 6
    assert rec["metric"].startswith("rows/sec (whole node), LSTM seq64")
    # value is the whole-job aggregate: global rows per step / seconds per step
    assert rec["value"] == pytest.approx(B * world / (rec["ms_per_step"] / 1000.0), rel=1e-3)
    assert rec["dtype"] == "fp32" and "rehearsal" in rec["data"]  # never mistaken for the benchmark
    assert rec["higher_is_better"] is True and rec["scaling"] == "weak"


def test_bench_self_spawns_ranks():
    """`python bench.py --gpus 4` with no launcher: the parent starts 4 ranks itself
    (torch.distributed.run on 127.0.0.1) and exactly one JSON line comes back, n_gpus 4."""
    B = 4
    rec = _run(4, "lstm", ["--batch", str(B), "--seq", "6", "--hidden", "16"], torchrun=False)
    assert rec["n_gpus"] == 4 and rec["world_size"] == 4 and rec["config"]["parallelism"] == "dp4"
    assert rec["config"]["global_batch"] == 4 * B and rec["backend"] == "gloo"


def test_bench_refuses_world_mismatch():
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="", WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "2", "--device", "cpu", "--steps", "1"],
                       capture_output=True, text=True, env=env, cwd=ROOT, timeout=300)
    assert r.returncode == 2 and not r.stdout.strip()


def test_bench_json_contract_mlp_dp2():
    rec = _run(2, "mlp", ["--batch", "64"])
    assert rec["config"]["global_batch"] == 128 and rec["n_gpus"] == 2


def test_bench_refuses_without_gpu():
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, "bench.py", "--steps", "1", "--warmup", "0"], capture_output=True,
                       text=True, env=env, cwd=ROOT, timeout=300)
    assert r.returncode == 2 and not r.stdout.strip()


def test_bench_secondary_configs_dp2():
    """BASELINE.json:8-10 ride in the headline's JSON line: a nested "secondary" object, one
    entry per config with its own steps, ms/step, rows/s (whole-job aggregate) and timed
    seconds; the headline value stays the LSTM's."""
    B = 4
    rec = _run(2, "lstm", ["--batch", str(B), "--seq", "6", "--hidden", "16", "--full", "--secondary",
                          "mlp,mlp_online,cnn"])
    assert rec["value"] == pytest.approx(B * 2 / (rec["ms_per_step"] / 1000.0), rel=1e-3)
    sec = rec["secondary"]
    assert set(sec) == {"mlp", "mlp_online", "cnn"}
    for m, v in sec.items():
        assert v["steps"] == 3 and v["warmup"] == 1 and v["global_batch"] == 2 * v["per_gpu_batch"]
        assert v["value"] == pytest.approx(v["global_batch"] / (v["ms_per_step"] / 1000.0), rel=1e-3), (m, v)
        assert v["timed_s"] == pytest.approx(v["ms_per_step"] * 3 / 1000.0, rel=1e-2)
        # round-5 VERDICT item 5: every secondary carries its OWN bucket's all-reduce time at
        # this world size (gloo here, RCCL on the GPU node) and its share of the step
        assert v["comm_ms"] is not None and v["comm_ms"] > 0, (m, v)
        assert v["grad_bucket_mb"] > 0 and v["comm_dtype"] == "fp32"
        assert v["comm_share"] == pytest.approx(v["comm_ms"] / v["ms_per_step"], rel=1e-2, abs=1e-3)
    assert rec["comm_ms"] is not None and rec["comm_ms"] > 0


def test_gpu_state_sampler_window_math():
    """utils/gpustate.py on a fake metrics table: sampled clock / power / temperature, the
    limiter residencies as fractions of the accumulation counter's delta, per-XCD clocks
    averaged, N/A placeholders skipped."""
    import time

    sys.path.insert(0, ROOT)
    from wellflow.utils.gpustate import GpuStateSampler

    n = {"k": 0}

    def fake(_h):
        n["k"] += 1
        k = n["k"]
        return {"current_gfxclks": [2000 + k, 2000 + k, "N/A"], "current_socket_power": 1000 + k,
                "temperature_hotspot": 70 + k % 3, "accumulation_counter": 100 * k,
                "ppt_residency_acc": 25 * k, "socket_thm_residency_acc": 0, "throttle_status": 1}

    s = GpuStateSampler.__new__(GpuStateSampler)
    s.period_s, s._h, s._get, s._samples, s._t0, s._thread = 0.005, object(), fake, [], None, None
    import threading

    s._stop = threading.Event()
    s.start()
    time.sleep(0.05)
    st = s.stop()
    assert st["samples"] >= 2
    assert 2000 < st["sclk_mhz"]["min"] <= st["sclk_mhz"]["max"] < 2000 + n["k"] + 1
    assert st["power_w"]["max"] > 1000 and 70 <= st["temp_hotspot_c"] <= 72
    assert st["throttle"]["ppt"] == 0.25 and st["throttle"]["socket_thm"] == 0.0
    assert st["throttle"]["throttle_status"] == 1
    off = GpuStateSampler.__new__(GpuStateSampler)
    off._h, off._thread = None, None
    assert not off.available and off.stop() is None


def test_bench_job_default_secondaries():
    """The submission API's own batches ride in the bench line too (CNN 20 windows, MLP and
    online MLP 256 rows): the secondary names map to (model, per-GPU batch)."""
    rec = _run(1, "lstm", ["--batch", "4", "--seq", "6", "--hidden", "16", "--full", "--secondary",
                           "cnn_b20,mlp_b256,mlp_online_b256"])
    sec = rec["secondary"]
    assert set(sec) == {"cnn_b20", "mlp_b256", "mlp_online_b256"}
    assert sec["cnn_b20"]["per_gpu_batch"] == 20 and "cnn" in sec["cnn_b20"]["metric"]
    assert sec["mlp_b256"]["per_gpu_batch"] == 256 and sec["mlp_online_b256"]["per_gpu_batch"] == 256
    assert all(v["value"] > 0 for v in sec.values())


def _bench_module():
    import importlib.util

    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def test_plain_run_is_the_headline_alone():
    """Everything besides the headline sits behind --full: a plain default run selects no
    secondary config and no parity pass, --full selects what the default line used to carry, and
    naming a secondary (or --parity on) without --full is refused, not silently dropped."""
    bench = _bench_module()
    assert bench._select_extras(False, "auto", "auto", True, 1, False) == ([], False)
    assert bench._select_extras(True, "auto", "auto", True, 1, False) == (list(bench.SECONDARY), True)
    assert bench._select_extras(True, "auto", "auto", True, 8, False) == (["mlp", "mlp_online", "cnn"], True)
    assert bench._select_extras(True, "auto", "auto", False, 1, False) == ([], False)  # another --model / shape
    assert bench._select_extras(True, "mlp,cnn", "none", True, 1, False) == (["mlp", "cnn"], False)
    assert bench._select_extras(True, "none", "on", False, 1, False) == ([], True)
    assert bench._select_extras(True, "auto", "on", True, 1, True) == (list(bench.SECONDARY), False)  # CPU rehearsal
    assert bench._select_extras(False, "none", "none", True, 1, False) == ([], False)
    for sec, par in (("mlp", "auto"), ("none", "on")):
        with pytest.raises(ValueError, match="--full"):
            bench._select_extras(False, sec, par, True, 1, False)
    with pytest.raises(ValueError, match="unknown"):
        bench._select_extras(True, "resnet", "auto", True, 1, False)
    r = subprocess.run([sys.executable, "bench.py", "--device", "cpu", "--secondary", "mlp"], capture_output=True,
                       text=True, env=dict(os.environ, CUDA_VISIBLE_DEVICES=""), cwd=ROOT, timeout=300)
    assert r.returncode == 2 and not r.stdout.strip() and "--full" in r.stderr


def test_bench_dump_outputs(tmp_path):
    """--dump-outputs DIR: what the timed step left its caller after the last of exactly --steps
    steps, as float32 .npy files; the inputs and initial weights are seeded, so a second run
    with the same arguments writes the same arrays (the fp32 CPU step is deterministic)."""
    import numpy as np

    outs = []
    for name in ("a", "b"):
        d = tmp_path / name
        rec = _run(1, "lstm", ["--batch", "4", "--seq", "6", "--hidden", "16", "--dump-outputs", str(d)])
        assert rec["steps"] == 3 and "secondary" not in rec and "parity" not in rec
        assert rec["dumped_outputs"]["dir"] == str(d)
        arrs = {f[:-4]: np.load(d / f) for f in sorted(os.listdir(d))}
        assert {"params", "loss"} <= set(arrs) == set(rec["dumped_outputs"]["elements"])
        for k, a in arrs.items():
            assert a.dtype == np.float32 and a.ndim == 1 and np.isfinite(a).all(), k
            assert rec["dumped_outputs"]["elements"][k] == [a.size, a.size]
        assert arrs["loss"][0] == pytest.approx(rec["train_loss"], rel=1e-5, abs=1e-6)  # float32 / 6 decimals
        outs.append(arrs)
    assert outs[0]["params"].size == 4 * 16 * (16 + 16) + 2 * 4 * 16 + 16 + 1  # torch LSTM + linear head
    for k in outs[0]:
        np.testing.assert_array_equal(outs[0][k], outs[1][k])


def test_dump_outputs_size_cap(tmp_path, monkeypatch):
    """Past 64 MB in all, an array above its share is written as a fixed seeded sample."""
    import numpy as np
    import torch

    bench = _bench_module()
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 4 * 300)
    big, small = torch.arange(1000.0), torch.arange(7.0)
    for d in ("a", "b"):
        w = bench._dump_outputs(str(tmp_path / d), {"big": big, "small": small})
        assert w == {"big": [150, 1000], "small": [7, 7]}
    a, b = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "b" / "big.npy")
    assert a.dtype == np.float32 and a.size == 150 and (np.diff(a) > 0).all()
    np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "small.npy"), small.numpy())


def test_small_launch_steps_and_dp_secondaries():
    """The headline times exactly --steps (<= 256 per launch); a secondary's raised window runs
    the Trainer's 256-step launches. Under a DP world the job-default secondaries are left out
    of the automatic set (they show one-GPU paths)."""
    import argparse
    import importlib.util

    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    assert bench._small_launch_steps(argparse.Namespace(min_timed_s=0.0, steps=20)) == 20
    assert bench._small_launch_steps(argparse.Namespace(min_timed_s=0.0, steps=1000)) == 256
    assert bench._small_launch_steps(argparse.Namespace(min_timed_s=0.1, steps=20)) == 256
    assert set(bench.SMALL_SECONDARY) <= set(bench.SECONDARY)
    assert bench._auto_secondary(True, 1) == list(bench.SECONDARY)
    assert bench._auto_secondary(True, 8) == ["mlp", "mlp_online", "cnn"]
    assert bench._auto_secondary(False, 1) == []
