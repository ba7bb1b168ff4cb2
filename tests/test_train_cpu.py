"""Trainer semantics, checkpoint/resume, submission contract (CPU, fp32 oracle path)."""
import os
import subprocess
import sys

import pytest
import torch

from wellflow.config import parse_argv
from wellflow.train.trainer import EarlyStopping

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = "well,field,t,whp,choke,glr,temp,water_cut,dsp,flow"
TYPES = "string,string,int,float,float,float,float,float,float,float"


def test_early_stopping_keras01_rule():
    es = EarlyStopping(patience=2)
    seq = [1.0, 0.9, 0.95, 0.96, 0.97]
    stops = [es.update(v) for v in seq]
    # after the best (0.9): wait 0 -> 1 -> 2, stop when wait >= patience is checked
    assert stops == [False, False, False, False, True]
    assert es.best == 0.9


def test_argv_contract_and_storage_path():
    cfg = parse_argv("cnn", ["a,b", "int,float", "b", "/data/out/"])
    assert cfg.data == "synth" and cfg.mdl_path() == "/data/out/models/cnn.mdl"
    assert (cfg.lr, cfg.momentum, cfg.decay, cfg.nesterov) == (0.001, 0.99, 1e-6, True)
    assert (cfg.batch_size, cfg.epochs, cfg.patience, cfg.loss) == (20, 1000, 10, "mae_clip")
    cfg = parse_argv("lstm", ["a,b", "int,float", "b", "/data/out", "/x.csv", "--epochs", "3"])
    assert cfg.data == "/x.csv" and cfg.epochs == 3 and cfg.mdl_path() == "/data/out/models/lstm.mdl"
    assert (cfg.seq_len, cfg.hidden) == (64, 512)


def _run_script(rel, args, env=None, cwd=None):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, rel), *args], capture_output=True,
                          text=True, env=e, cwd=cwd, timeout=300)


def test_cnn_script_stdout_contract_and_mdl(tmp_path):
    r = _run_script("Artificial intelligence models/Static neural network models/cnn.py",
                    [NAMES, TYPES, "flow", str(tmp_path) + "/", "--epochs", "2", "--synth-wells", "3",
                     "--synth-steps", "150", "--device", "cpu"])
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().splitlines()
    assert lines[0].startswith("StructType([")
    assert lines[1] == "Categorical variables: well, field"
    assert lines[-2].startswith("Time elapsed: ") and lines[-2].endswith(" s")
    assert lines[-1].startswith("Testing set loss: ")
    assert (tmp_path / "models" / "cnn.mdl").exists()


def test_resume_after_injected_fault(tmp_path):
    args = [NAMES, TYPES, "flow", str(tmp_path), "--epochs", "4", "--synth-wells", "3",
            "--synth-steps", "120", "--device", "cpu", "--batch-size", "32"]
    rel = "Artificial intelligence models/Static neural network models/mlp.py"
    # count steps per epoch from a clean run
    ok = _run_script(rel, args)
    assert ok.returncode == 0, ok.stderr
    for p in (tmp_path / "models").iterdir():
        p.unlink()
    r = _run_script(rel, args, env={"WELLFLOW_FAIL_AT_STEP": "9"})
    assert r.returncode != 0 and "injected fault" in r.stderr
    assert (tmp_path / "models" / "mlp.ckpt").exists()
    r2 = _run_script(rel, args + ["--resume"])
    assert r2.returncode == 0, r2.stderr
    assert "Resumed from" in r2.stdout
    # both runs end with the same number of epochs in history
    from wellflow.utils.checkpoint import load_state

    st = load_state(str(tmp_path / "models" / "mlp.ckpt"))
    assert st["epoch"] == 4


def test_online_and_gilbert_jobs(tmp_path):
    from wellflow.train.job import run_job

    out = run_job("mlp_online", [NAMES, TYPES, "flow", str(tmp_path), "--epochs", "1", "--synth-wells",
                                 "4", "--synth-steps", "200", "--online-chunk", "128", "--device", "cpu",
                                 "--mlp-hidden", "32,16"], log=lambda *a, **k: None)
    assert out["epochs"] >= 3 and out["test_loss"] == out["test_loss"]
    # second submission warm-starts from the saved dynamic model
    msgs = []
    run_job("mlp_online", [NAMES, TYPES, "flow", str(tmp_path), "--epochs", "1", "--synth-wells", "4",
                           "--synth-steps", "200", "--online-chunk", "128", "--device", "cpu",
                           "--mlp-hidden", "32,16"], log=lambda *a, **k: msgs.append(str(a[0]) if a else ""))
    assert any(m.startswith("Warm start from") for m in msgs)
    g = run_job("gilbert", [NAMES, TYPES, "flow", str(tmp_path)], log=lambda *a, **k: None)
    assert g["test_mse"] > 0 and (tmp_path / "models" / "gilbert.mdl").exists()


def test_lstm_job_learns_on_cpu(tmp_path):
    from wellflow.train.job import run_job

    out = run_job("lstm", [NAMES, TYPES, "flow", str(tmp_path), "--epochs", "6", "--synth-wells", "4",
                           "--synth-steps", "160", "--hidden", "128", "--seq-len", "16",
                           "--batch-size", "64", "--device", "cpu"], log=lambda *a, **k: None)
    h = out["history"]
    assert h["val_loss"][-1] < h["val_loss"][0]


def test_evaluate_with_native_window_prefetcher_matches_plain_gather(monkeypatch):
    """Trainer.evaluate on a host-resident window set gathers chunk k+1 in the native
    background prefetcher (csrc/runtime, wf_prefetch_*) while chunk k is evaluated; the result
    must equal the plain per-chunk gather (WELLFLOW_NATIVE_IO=0)."""
    import numpy as np

    from wellflow.data import native
    from wellflow.data.features import SeriesWindows
    from wellflow.models.base import TorchEngine
    from wellflow.models.lstm import LSTMRegressor
    from wellflow.parallel.dist import DistContext
    from wellflow.train.trainer import Trainer

    if not native.available():
        pytest.skip("native runtime not built")
    rng = np.random.default_rng(3)
    T, F = 12, 5
    rows = rng.standard_normal((700, F)).astype(np.float32)
    starts = np.arange(0, 700 - T, 2, dtype=np.int64)
    X = SeriesWindows(rows, starts, T)
    Y = rng.standard_normal(len(starts)).astype(np.float32)
    torch.manual_seed(0)
    eng = TorchEngine(LSTMRegressor(F, hidden=16))
    cfg = type("Cfg", (), {"loss": "mse", "clip": 6.0, "batch_size": 64, "patience": 3})()
    tr = Trainer(cfg, eng, None, DistContext(), "t")
    calls = []
    orig = native.Prefetcher.wait
    monkeypatch.setattr(native.Prefetcher, "wait", lambda self, s: calls.append(s) or orig(self, s))
    with_pf = tr.evaluate(X, Y, chunk=50)
    assert len(calls) == -(-len(starts) // 50)  # every chunk came through the prefetcher
    monkeypatch.setenv("WELLFLOW_NATIVE_IO", "0")
    plain = tr.evaluate(X, Y, chunk=50)
    assert with_pf == pytest.approx(plain, rel=1e-6)


def test_stream_chunks_are_balanced():
    """chunk_bounds: the chunks of a pass hold equal full-batch counts (+-1) and every full
    batch is kept (round-4 VERDICT item 8: an 8 + 1 split made every other chunk pay the
    fixed per-chunk cost over one step)."""
    import numpy as np

    from wellflow.train.online import chunk_bounds, rank_batches, rank_shard

    for n, b, w in [(2_457_600, 262_144, 1), (2_457_600, 65_536, 4), (100_000, 256, 2), (20_485, 256, 1),
                    (1000, 256, 8), (121 * 512, 256, 2), (37 * 100 + 5, 100, 1), (9 * 4096 + 7, 4096, 1)]:
        unit = b * w
        starts = chunk_bounds(n, 8 * unit, unit)
        ends = starts[1:] + [n]
        full = [(e - s) // unit for s, e in zip(starts, ends)]
        assert starts[0] == 0 and all(e > s for s, e in zip(starts, ends))
        if n >= unit:
            assert max(full) - min(full) <= 1 and max(full) <= 8, (n, b, w, full)
            assert sum(full) == n // unit  # no full batch lost to the chunking
    X = np.arange(1000 * 2, dtype=np.float32).reshape(1000, 2)
    Y = np.arange(1000, dtype=np.float32)
    seen = []
    for r in range(2):  # the shards of 2 ranks cover exactly the chunks' per-rank rows
        Xs, Ys, table = rank_shard(X, Y, 8 * 64 * 2, r, 2, unit=64 * 2)
        for off, n_rows, per_rank in table:
            for xb, yb in rank_batches(Xs[off : off + per_rank], Ys[off : off + per_rank], 64, 0, 1):
                seen.extend(yb.tolist())
    assert len(seen) == len(set(seen)) == (1000 // 128) * 128


def test_resume_with_other_layout_fails_clearly(tmp_path):
    """A checkpoint whose flat parameter layout differs from the engine's (another hidden
    size, or an older padding) is refused with a message naming both layouts (round-4 ADVICE)."""
    import pytest as _pytest

    from wellflow.train.job import run_job
    from wellflow.utils.checkpoint import load_state

    base = [NAMES, TYPES, "flow", str(tmp_path), "--epochs", "1", "--synth-wells", "3",
            "--synth-steps", "120", "--device", "cpu", "--batch-size", "32", "--verbose", "0"]
    run_job("mlp", base, log=lambda *a, **k: None)
    st = load_state(str(tmp_path / "models" / "mlp.ckpt"))
    assert st["layout"]["numel"] == st["params"].numel()
    with _pytest.raises(ValueError, match="layout does not match"):
        run_job("mlp", base + ["--mlp-hidden", "64,64", "--resume"], log=lambda *a, **k: None)


def test_auto_online_chunk_is_sized_in_rows():
    """Round-5 ADVICE: the auto stream chunk (online_chunk 0) is sized in ROWS, not in
    mini-batches: at the job default batch of 256 a chunk is no longer 8,192 rows per rank (which
    made validation / checkpoint I/O dominate and let patience 5 stop after ~40K rows)."""
    from wellflow.train.job import ONLINE_CHUNK_ROWS, auto_online_chunk

    # a 15 M-row stream on one rank at batch 256: 2M-row chunks (the round-4 size), whole batches
    c = auto_online_chunk(256, 15_000_000, 1)
    assert c == ONLINE_CHUNK_ROWS and c % 256 == 0
    # at DP=8 the chunk covers every rank's share
    assert auto_online_chunk(256, 15_000_000, 8) == 8 * ONLINE_CHUNK_ROWS
    # a short stream still gets >= 4 validation points per pass ...
    c = auto_online_chunk(256, 400_000, 1)
    assert 400_000 // c >= 4 and c % 256 == 0
    # ... and never fewer than 32 mini-batches per chunk (262,144-row batches: 32 x B)
    assert auto_online_chunk(262_144, 15_000_000, 1) == 32 * 262_144
    assert parse_argv("mlp_online", ["a", "float", "a", "/tmp/"]).online_chunk == 0  # 0 = auto


def test_sliced_epochs_bound_the_graph_count():
    """Round-5 ADVICE: the pre-permuted (sliced) epoch path keys its graphs by step offset, so it
    is taken only up to MAX_SLICED_STEPS steps per epoch; longer epochs use the row-indexed path,
    whose graphs are keyed by the group length only."""
    import inspect

    from wellflow.train import trainer

    assert 16 <= trainer.MAX_SLICED_STEPS <= 512
    src = inspect.getsource(trainer.Trainer.fit)
    assert "MAX_SLICED_STEPS" in src and "_permuted" in src


INF = float("inf")


def _singles(lo, hi):
    return [(s, 1) for s in range(lo, hi)]


def test_pass_schedule_literals():
    """The replay path's launches, row by row as the loop issued them before the schedule was a
    function of its own (eager_steps = 2: the first 4 - calls steps of a runner are singles), the
    balanced group length, and the K-step path's launches."""
    from wellflow.train.trainer import SMALL_STEPS_PER_LAUNCH as K, group_len, pass_schedule, small_schedule

    rows = [  # steps, graph_steps, n, aligned, runner calls at entry, budget, schedule
        (9, 8, 9, True, 0, INF, _singles(0, 9)),
        (9, 8, 9, True, 9, INF, [(0, 9)]),
        (20, 8, 10, True, 0, INF, _singles(0, 10) + [(10, 10)]),
        (20, 8, 10, False, 0, INF, _singles(0, 4) + [(4, 10)] + _singles(14, 20)),
        (20, 8, 10, False, 20, INF, [(0, 10), (10, 10)]),
        (20, 8, 10, True, 20, 17, [(0, 10)] + _singles(10, 17)),
        (13, 4, 5, True, 2, INF, _singles(0, 5) + [(5, 5)] + _singles(10, 13)),
        (13, 4, 5, False, 2, INF, _singles(0, 2) + [(2, 5), (7, 5)] + _singles(12, 13)),
    ]
    for steps, gs, n, aligned, calls, budget, want in rows:
        assert group_len(steps, gs, True) == n
        assert pass_schedule(steps, n, max(0, 4 - calls), aligned, budget) == want, (steps, gs, aligned, calls)
    assert [group_len(s, 8, True) for s in (12, 20, 2)] == [6, 10, 2]  # Python's round(): 1.5 -> 2, 2.5 -> 2
    assert group_len(20, 8, False) == 1 and group_len(1, 8, True) == 8 and group_len(0, 8, True) == 8
    # a pass entered with the budget spent: one single step on the replay path, none on the K-step path
    assert pass_schedule(5, 1, 0, False, 0) == [(0, 1)] and pass_schedule(5, 5, 0, True, -2) == [(0, 1)]
    assert small_schedule(5, 0) == [] and small_schedule(5, -2) == [] and small_schedule(0) == []
    assert small_schedule(2 * K + 88) == [(0, K), (K, K), (2 * K, 88)]
    assert small_schedule(2 * K + 88, K + 44) == [(0, K), (K, 44)] and small_schedule(3, 300) == [(0, 3)]


def test_pass_schedule_properties():
    """What fixes the replay schedule uniquely, over steps x group length x warm-up x alignment x
    budget: the launches tile the pass from step 0 up to min(steps, budget), each is one step or a
    whole group, and a group is taken exactly where one is allowed."""
    from wellflow.train.trainer import group_len, pass_schedule

    for steps in range(41):
        for gs in (1, 2, 3, 4, 8):
            n = group_len(steps, gs, True)
            for warm in range(7):
                for aligned in (True, False):
                    for budget in (1, 5, 17, INF):
                        at = 0
                        for s, c in pass_schedule(steps, n, warm, aligned, budget):
                            case = (steps, n, warm, aligned, budget, s, c)
                            assert s == at and c in (1, n), case  # contiguous from 0, no overlap
                            allowed = (n > 1 and s >= warm and s + n <= steps and s + n <= budget
                                       and (not aligned or s % n == 0))
                            assert (c == n) if allowed else (c == 1), case
                            at += c
                        assert at == min(steps, budget), (steps, n, warm, aligned, budget)


class _RecordingRunner:
    """Stands in for StepRunner: at each call it reads ``inputs`` as the captured step would and
    records the dataset rows of every step of the launch (Y[i] == i, static index buffers
    resolved at call time)."""
    eager_steps, loss_acc = 2, None

    def __init__(self, inputs):
        self.inputs, self.calls, self.seen, self.prepared = inputs, 0, [], []

    def _rows(self, key):
        x, y, *rows = self.inputs(key)
        return [int(v) for v in (y[rows[0]] if rows else y)]

    def run(self, key=0):
        self.calls += 1
        self.seen.append(self._rows(key))

    def run_many(self, n, key=0):
        self.calls += n
        self.seen.extend(self._rows((key, i)) for i in range(n))

    def prepare_many(self, n, key=0):
        self.prepared.append((n, key, len(self.seen), [self._rows((key, i)) for i in range(n)]))
        return True

    def take_loss(self):
        return 0.0


@pytest.mark.parametrize("budget", [INF, 7])
@pytest.mark.parametrize("source,n,aligned,warm", [("sliced", 5, True, 5), ("indexed", 5, False, 2),
                                                   ("gathered", 1, False, 0)])
def test_each_step_trains_on_its_rows_whatever_the_schedule(source, n, aligned, warm, budget):
    """Step j of a pass trains on rows order[j*b : (j+1)*b] of the dataset, through each batch
    source and a schedule that mixes single steps and groups; the step count advances by the
    steps run, max_steps ends the pass, and the sliced path prepares each aligned group's graph
    exactly once, after the warm-up steps."""
    from wellflow.parallel.dist import DistContext
    from wellflow.train import trainer as T

    b, steps, N = 4, 13, 64
    order = torch.randperm(N, generator=torch.Generator().manual_seed(5))[: steps * b + 2]
    X, Y = torch.arange(N * 3, dtype=torch.float32).reshape(N, 3), torch.arange(N, dtype=torch.float32)
    idx, ordbuf = torch.zeros(b, dtype=torch.long), torch.zeros(n * b, dtype=torch.long)
    if source == "sliced":
        inputs, stage = T.sliced_source(X[order], Y[order], b)
    elif source == "indexed":
        inputs, stage = T.indexed_source(X, Y, order, b, idx, ordbuf)
    else:
        inputs, stage = T.gathered_source(X, Y, order, b, idx)
    cfg = type("Cfg", (), {"patience": 3, "fail_at_step": -1, "max_steps": 0 if budget == INF else budget})()
    eng = type("Eng", (), {"device": torch.device("cpu")})()
    tr = T.Trainer(cfg, eng, None, DistContext(device="cpu"), "t")
    run = _RecordingRunner(inputs)
    launches = T.pass_schedule(steps, n, warm, aligned, budget)
    if n > 1 and budget == INF:
        assert {c for _, c in launches} == {1, n}  # singles and groups
    loss, rows, dt, host = tr.run_pass(run, launches, T.replay_launcher(run, stage, n, warm, steps, aligned), b)
    ran = min(steps, budget)
    want = [order[j * b : (j + 1) * b].tolist() for j in range(steps)]
    assert run.seen == want[:ran]
    assert tr.global_step == ran == run.calls and rows == ran * b and dt > 0 and host > 0
    if source == "sliced":
        assert [p[:3] for p in run.prepared] == [(5, 0, warm), (5, 5, warm)]
        assert [p[3] for p in run.prepared] == [want[0:5], want[5:10]]
    else:
        assert run.prepared == []


def test_metrics_file_has_one_record_per_epoch_or_chunk(tmp_path):
    """--metrics FILE: one JSON line per epoch (mlp) and per stream chunk (mlp_online), as
    config.py documents, with ``epoch`` counting up from 1."""
    import json

    from wellflow.train.job import run_job

    base = [NAMES, TYPES, "flow", str(tmp_path), "--synth-wells", "4", "--synth-steps", "200", "--device", "cpu",
            "--mlp-hidden", "32,16", "--verbose", "0"]
    for model, extra in (("mlp_online", ["--epochs", "1", "--online-chunk", "128"]), ("mlp", ["--epochs", "3"])):
        path = tmp_path / f"{model}.jsonl"
        out = run_job(model, base + extra + ["--metrics", str(path)], log=lambda *a, **k: None)
        recs = [json.loads(ln) for ln in path.read_text().splitlines()]
        assert out["epochs"] >= 3 and [r["epoch"] for r in recs] == list(range(1, out["epochs"] + 1))
        assert [r["loss"] for r in recs] == out["history"]["loss"]


def test_writeback_skips_sync_only_when_the_fused_update_covers_the_optimizer():
    """StepRunner leaves out sync_weights only when the engine's fused optimizer launch will
    actually run for this optimizer (round-5 ADVICE: an LSTM engine with a shadow-writing Adam
    fell back to the plain update and trained on stale compute copies)."""
    import torch

    from wellflow.models.base import Engine
    from wellflow.parallel.dist import DistContext
    from wellflow.train.step import StepRunner

    class Eng(Engine):
        device = torch.device("cpu")
        grads = torch.zeros(4)

        def __init__(self, ok):
            self.ok = ok

        def fused_update_ok(self, opt):
            return self.ok

        def forward_backward(self, x, y, grad_scale, zero_grads=True, loss_into=None):
            return torch.zeros(1)

    class Opt:
        shadow = None
        zero_grads = False

        def __init__(self, eng):
            self.writeback = eng

    for ok in (True, False):
        eng = Eng(ok)
        run = StepRunner(eng, Opt(eng), DistContext(device="cpu"), 1.0, lambda k: (None, None), graph=False)
        assert run.fused_shadow is ok


def test_torch_engine_satisfies_every_engine_default():
    """TorchEngine adds nothing to the optional part of the contract: every capability flag,
    attribute and method has the Engine default, and forward_backward takes ``loss_into`` with
    the native engines' meaning (the batch loss added to the accumulator, which is returned)."""
    from wellflow.models.base import Engine, TorchEngine
    from wellflow.models.mlp import MLPRegressor
    from wellflow.optim.flat import FlatAdam

    torch.manual_seed(0)
    eng = TorchEngine(MLPRegressor(5, (8, 8)))
    assert isinstance(eng, Engine)
    for name in ("native", "row_indexed", "window_indexed"):
        assert getattr(eng, name) is False
    for name in ("input_dtype", "B", "rng", "lay", "small", "writeback_update"):
        assert getattr(eng, name) is None
    for name in ("to_input_format", "gather_rows", "sync_weights", "check_device_errors", "persistent_stats",
                 "small_steps_reason", "fused_steps", "fused_update_kwargs", "fused_update_ok",
                 "update_refreshes_operands"):
        assert getattr(type(eng), name) is getattr(Engine, name), name
    X = torch.randn(6, 5)
    assert eng.to_input_format(X) is X
    out = torch.empty(3, 5)
    eng.gather_rows(X, torch.tensor([4, 0, 2]), out)
    assert torch.equal(out, X[[4, 0, 2]])
    assert eng.sync_weights() is None and eng.check_device_errors() is None and eng.persistent_stats() == {}
    opt = FlatAdam(eng.params, eng.grads)
    why = eng.small_steps_reason(4, opt, X)
    assert isinstance(why, str) and why
    with pytest.raises(RuntimeError, match="TorchEngine.fused_steps: " + why):
        eng.fused_steps(X, X[:, 0], 4, 1, opt, 1.0)
    assert eng.fused_update_kwargs("adam") == {} and eng.fused_update_kwargs("sgd") == {}
    assert eng.update_refreshes_operands(opt) is False
    assert eng.update_refreshes_operands(FlatAdam(eng.params, eng.grads, writeback=eng)) is False
    y = torch.randn(6)
    ls = eng.forward_backward(X, y, 1.0 / 6)
    g = eng.grads.clone()
    acc = torch.full((1,), 2.0)
    assert eng.forward_backward(X, y, 1.0 / 6, loss_into=acc) is acc
    assert torch.equal(acc, 2.0 + ls) and torch.equal(eng.grads, g)


def test_cpu_job_checkpoint_keeps_the_layout_tag(tmp_path):
    """The .ckpt of a CPU job carries the layout tag this literal records (taken from a run before
    the engines had a base class), so older checkpoints resume and newer ones read the same."""
    from wellflow.train.job import run_job
    from wellflow.utils.checkpoint import load_state

    run_job("mlp", [NAMES, TYPES, "flow", str(tmp_path), "--epochs", "1", "--synth-wells", "3", "--synth-steps", "120",
                    "--device", "cpu", "--batch-size", "32", "--verbose", "0"], log=lambda *a, **k: None)
    st = load_state(str(tmp_path / "models" / "mlp.ckpt"))
    assert st["layout"] == {"engine": "TorchEngine", "numel": 69633, "layout": None}


def test_small_steps_path_eligibility(capfd, monkeypatch):
    """train.trainer.small_steps_path, the one K-steps-per-launch decision of Trainer.train_steps
    and fit_online: not eligible with two ranks, with fault injection (the engine is not even
    asked) or when the engine has no such kernel; eligible when the engine has no objection; and
    when clipping is the engine's only objection, that is said once however often it is asked."""
    from wellflow.models import base
    from wellflow.train.trainer import small_steps_path

    monkeypatch.setattr(base, "_NOTED", set())
    asked = []

    class Eng(base.Engine):
        def __init__(self, why):
            self.why = why

        def small_steps_reason(self, B, opt=None, X=None):
            asked.append(B)
            return self.why

    def ctx(world):
        return type("Ctx", (), {"world_size": world})()

    def cfg(fail):
        return type("Cfg", (), {"fail_at_step": fail})()

    assert small_steps_path(Eng(None), None, ctx(1), cfg(-1), 32, None) == (True, None)
    assert asked == [32]
    assert small_steps_path(Eng(None), None, ctx(2), cfg(-1), 32, None) == (False, None)
    assert small_steps_path(Eng(None), None, ctx(1), cfg(0), 32, None) == (False, None)
    assert small_steps_path(Eng(None), None, ctx(1), cfg(7), 32, None) == (False, None)
    assert asked == [32]  # more than one rank / fault injection: decided without the engine
    ok, why = small_steps_path(base.Engine(), None, ctx(1), cfg(-1), 32, None)  # no kernel at all
    assert ok is False and isinstance(why, str) and why
    assert small_steps_path(Eng("batch 33"), None, ctx(1), cfg(-1), 33, None) == (False, "batch 33")
    assert capfd.readouterr().err == ""
    for _ in range(3):
        assert small_steps_path(Eng(base.CLIP_STEPS_REASON), None, ctx(1), cfg(-1), 32, None) == \
            (False, base.CLIP_STEPS_REASON)
    err = capfd.readouterr().err
    assert err.count(base.CLIP_STEPS_REASON) == 1 and "Eng" in err and "B=32" in err, err
