"""Resume on the native engines: a restore brings back every carried buffer bit for bit, and the
run after it is the run that was never interrupted.

What a job carries on the device is declared in wellflow/train/state_ref.py (four classes; the
carried and rebuilt ones are compared here, by bit pattern). Each case builds engine, optimizer and
Trainer the way train/job.py does and trains through Trainer.train_steps on a resident dataset,
rows taken through an order tensor (the route of every epoch; K steps per launch where the engine
has a small-batch kernel, else two eager steps, the capture and replays), so the device counters
are advanced by launches and replays, not by the host. Three engines per case:

* donor    trains N steps, is saved (Trainer.state_dict -> checkpoint.save_state / load_state),
           and trains on;
* twin     same seed, same steps, never saved: what two uninterrupted runs differ by;
* restored a FRESH engine + optimizer + Trainer that loads the checkpoint, then trains the same
           three further steps, through its own warm-up, capture and replays.

Nothing here writes to a sync word, a ticket or a STAT block, poisons scratch, or runs a kernel on
state that was altered: the negative controls only load and compare.
"""
import contextlib
import dataclasses

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
MORE = 3  # steps after the restore


@dataclasses.dataclass(frozen=True)
class Case:
    id: str
    model: str
    B: int
    route: str                    # "small": K steps per launch | "graph": one-step graphs | "graph+many"
    passes: tuple = (5,)          # steps per Trainer.train_steps call before the save
    F: int = 16
    T: int = 16
    H: int = 128
    cfg: tuple = ()               # RunConfig overrides
    env: tuple = ()
    persistent: bool | None = None  # LSTM: the persistent kernels ran
    fused: bool | None = None       # CNN: the fused kernels (False: im2col + GEMMs)
    refuses: str = ""               # a word of the small-batch kernel's reason, where it refuses


CLIP = (("clipnorm", 0.05), ("clipvalue", 0.01))
CASES = [
    Case("mlp_b256_small", "mlp", 256, "small"),
    # a grouped replay cannot start before the fifth step (two eager steps, the capture, one checked
    # replay), so five steps hold none: this case saves after two passes of four, the second of
    # which is ONE four-step replay (StepRunner.run_many), as every epoch after the first is
    Case("mlp_b4096_graphs", "mlp", 4096, "graph+many", passes=(4, 4), refuses="batch 4096"),
    Case("mlp_f40_wide", "mlp", 256, "graph", F=40, refuses="shape F=40"),
    Case("lstm_b64_persistent", "lstm", 64, "graph", persistent=True),
    Case("lstm_b40_per_step", "lstm", 40, "graph", persistent=False),
    Case("lstm_f100_kx128", "lstm", 64, "graph", F=100, persistent=True),
    Case("cnn_b20_small", "cnn", 20, "small", fused=True),
    Case("cnn_b512_graphs", "cnn", 512, "graph", fused=True, refuses="batch 512"),
    Case("cnn_b64_gemm", "cnn", 64, "graph", fused=False, env=(("WELLFLOW_CNN_FUSED", "0"),),
         refuses="not covered by the fused kernels"),
    Case("mlp_b256_adam_clip", "mlp", 256, "graph", cfg=CLIP, refuses="gradient clipping"),
    Case("cnn_b20_sgd_clip", "cnn", 20, "graph", fused=True, cfg=CLIP, refuses="gradient clipping"),
]
BY_ID = {c.id: c for c in CASES}


def _config(case: Case, storage: str):
    from wellflow.config import MODEL_DEFAULTS, RunConfig

    cfg = RunConfig(model=case.model, **MODEL_DEFAULTS[case.model])
    cfg.storage_path, cfg.device, cfg.verbose, cfg.seed = storage, "cuda", 0, 7
    cfg.batch_size, cfg.hidden, cfg.seq_len = case.B, case.H, case.T
    if case.model == "cnn":  # the reference layout and optimizer: SGD-Nesterov, decay 1e-6, dropout 0.5
        assert (cfg.optimizer, cfg.nesterov, cfg.decay, cfg.dropout) == ("sgd", True, 1e-6, 0.5)
    for k, v in case.cfg:
        assert hasattr(cfg, k)
        setattr(cfg, k, v)
    return cfg


def _dataset(case: Case, steps: int):
    """(X, Y, n_features, n_outputs) on the device: ``steps`` batches of distinct rows, one fixed
    sequence for all three engines."""
    from wellflow.data.features import SeriesWindows

    g = torch.Generator().manual_seed(11)
    n = steps * case.B
    if case.model == "mlp":
        X = torch.randn(n, case.F, generator=g)
        Y = torch.tanh(X[:, :4].sum(1)) + 0.1 * torch.randn(n, generator=g)
        return X.to(DEV), Y.to(DEV), case.F, 1
    if case.model == "lstm":
        rows = torch.randn(n + case.T, case.F, generator=g)
        Y = torch.tanh(rows[case.T - 1 : case.T - 1 + n, :4].sum(1))
        W = SeriesWindows(rows.numpy(), torch.arange(n).numpy(), case.T).to(DEV)
        return W, Y.to(DEV), case.F, 1
    X = torch.randn(n, 48, 1, generator=g)
    Y = torch.randn(n, 12, generator=g) + X[:, :12, 0]
    return X.to(DEV), Y.to(DEV), 1, 12


def _build(case: Case, cfg, n_features: int, n_out: int):
    """Engine, optimizer and Trainer exactly as train/job.py run_config builds them."""
    from wellflow.models import registry
    from wellflow.parallel.dist import DistContext
    from wellflow.train.job import _optimizer
    from wellflow.train.trainer import Trainer

    eng, _ = registry.build_engine(case.model, cfg, n_features, n_out, case.B, DEV, True, seed=cfg.seed)
    opt = _optimizer(cfg, eng)
    return Trainer(cfg, eng, opt, DistContext(device=DEV), case.model, n_outputs=n_out, log=lambda *a, **k: None)


def _train(tr, X, Y, b: int, first: int, steps: int) -> float:
    """One Trainer.train_steps pass over batches first .. first + steps - 1 -> its mean loss."""
    order = torch.arange(first * b, (first + steps) * b, device=DEV)
    loss = tr.train_steps(X, Y, b, order)[0]
    tr.eng.check_device_errors()
    return loss


def _state(tr) -> dict:
    from wellflow.train.state_ref import device_state

    return device_state(tr.eng, tr.opt)


@contextlib.contextmanager
def _held_back(obj, attr: str, stand_in):
    """``obj.attr`` replaced for the duration of a load, so the load's write to it is lost."""
    keep = getattr(obj, attr)
    setattr(obj, attr, stand_in)
    try:
        yield
    finally:
        setattr(obj, attr, keep)


def _controls(case: Case, cfg, nf: int, no: int, sd: dict, donor: dict) -> dict:
    """{restoration skipped: names compare_states reports against the donor}. Compare only."""
    from wellflow.train.state_ref import compare_states

    out = {}
    moment = "vel" if case.model == "cnn" else "m"
    for what in ("sync_weights", "step_dev", moment) + (("rng",) if case.model == "cnn" else ()):
        tr = _build(case, cfg, nf, no)
        if what == "sync_weights":
            with _held_back(tr.eng, "sync_weights", lambda: None):
                tr.load_state_dict(sd)
        elif what == "step_dev":  # (the optimizers write the device counter only where they have one)
            with _held_back(tr.opt, "step_dev", None):
                tr.load_state_dict(sd)
        elif what == "rng":  # (Trainer.load_state_dict fills the counter only where the engine has one)
            with _held_back(tr.eng, "rng", None):
                tr.load_state_dict(sd)
        else:  # the moment is copied into a stand-in: the optimizer's own stays at zero
            with _held_back(tr.opt, what, torch.empty_like(getattr(tr.opt, what))):
                tr.load_state_dict(sd)
        out[what] = compare_states(donor, _state(tr))
        del tr
    return out


def _run_case(case: Case, tmp, monkeypatch) -> dict:
    from wellflow.train.state_ref import images, unclassified
    from wellflow.train.trainer import small_steps_path
    from wellflow.utils import checkpoint

    for k, v in case.env:
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("WELLFLOW_GRAPH_STEPS", "8")
    N, b = sum(case.passes), case.B
    cfg = _config(case, str(tmp) + "/")
    X, Y, nf, no = _dataset(case, N + MORE)
    donor, twin = _build(case, cfg, nf, no), _build(case, cfg, nf, no)
    X = donor.eng.to_input_format(X) if torch.is_tensor(X) else X  # (as Trainer.fit keeps it resident)
    res = {"N": N, "losses": {}, "states": {}}
    for tr in (donor, twin):
        at = 0
        for steps in case.passes:
            _train(tr, X, Y, b, at, steps)
            at += steps
    # ---- the donor at save time
    eng, opt = donor.eng, donor.opt
    res["small"], res["why"] = small_steps_path(eng, opt, donor.ctx, cfg, b, X)
    res["graphs"] = list(donor._runners[1].graphs)
    res["fused"] = getattr(eng, "fused", None)
    res["persistent"] = (getattr(eng, "last_forward_persistent", None), getattr(eng, "last_backward_persistent", None))
    res["unclassified"] = unclassified(eng, opt)
    res["images"] = images(eng)
    res["global_step"] = donor.global_step
    res["steps_taken"] = opt.steps_taken
    res["rng"] = None if eng.rng is None else int(eng.rng.item())
    res["ticket"] = float(opt.step_dev[1].item())
    res["states"]["donor", 0], res["states"]["twin", 0] = _state(donor), _state(twin)
    path = str(tmp / "state.ckpt")
    checkpoint.save_state(path, donor.state_dict())
    sd = checkpoint.load_state(path)
    # ---- a fresh engine, as a resume gets it
    restored = _build(case, cfg, nf, no)
    restored.load_state_dict(sd)
    res["states"]["restored", 0] = _state(restored)
    res["restored"] = {"global_step": restored.global_step, "steps_taken": restored.opt.steps_taken,
                       "ticket": float(restored.opt.step_dev[1].item()),
                       "rng": None if restored.eng.rng is None else int(restored.eng.rng.item()),
                       "clip_factor": float(restored.opt.clip_state[0].item()),
                       "clips": (restored.opt.clipnorm, restored.opt.clipvalue)}
    res["controls"] = _controls(case, cfg, nf, no, sd, res["states"]["donor", 0])
    # ---- three more steps, one pass each, so that the state can be read after every step
    for j in range(1, MORE + 1):
        for who, tr in (("donor", donor), ("twin", twin), ("restored", restored)):
            res["losses"][who, j] = _train(tr, X, Y, b, N + j - 1, 1)
            res["states"][who, j] = _state(tr)
    res["restored_graphs"] = list(restored._runners[1].graphs)
    res["restored_small"] = small_steps_path(restored.eng, restored.opt, restored.ctx, cfg, b, X)[0]
    res["restored_end"] = (restored.global_step, restored.opt.steps_taken,
                           None if restored.eng.rng is None else int(restored.eng.rng.item()))
    return res


_RESULTS: dict = {}


@pytest.fixture
def result(request, tmp_path_factory):
    """The case's three runs, made once and shared by the tests below (read only)."""
    cid = request.param
    if cid not in _RESULTS:
        with pytest.MonkeyPatch.context() as mp:
            _RESULTS[cid] = _run_case(BY_ID[cid], tmp_path_factory.mktemp(cid), mp)
    return BY_ID[cid], _RESULTS[cid]


IDS = [c.id for c in CASES]


@pytest.mark.parametrize("result", IDS, indirect=True)
def test_route_taken(result):
    case, r = result
    assert r["unclassified"] == []
    if case.route == "small":
        assert r["small"] and r["why"] is None and r["graphs"] == [], (r["why"], r["graphs"])
        assert r["restored_small"] and r["restored_graphs"] == []
    else:
        assert not r["small"] and case.refuses in (r["why"] or ""), r["why"]
        assert 0 in r["graphs"] and 0 in r["restored_graphs"], (r["graphs"], r["restored_graphs"])
        many = [k for k in r["graphs"] if isinstance(k, tuple) and k[0] == "many"]
        assert many == ([("many", 0, 4)] if case.route == "graph+many" else []), r["graphs"]
    if case.fused is not None:
        assert r["fused"] is case.fused
        assert r["images"] == (["WcA", "WdB", "WdF"] if case.fused else ["shadow"])
    if case.persistent is not None:
        assert r["persistent"] == (case.persistent, case.persistent), r["persistent"]
        assert r["images"] == ["WhhT", "Wp"]
    if case.model == "mlp":
        assert r["images"] == ["shadow", "w2t"]


@pytest.mark.parametrize("result", IDS, indirect=True)
def test_restore_is_exact_buffer_by_buffer(result):
    from wellflow.train.state_ref import compare_states

    case, r = result
    N = r["N"]
    # the donor at save time: launches and replays advanced the device counters, in step with the host's
    assert r["global_step"] == N and r["steps_taken"] == N and r["ticket"] == 0.0, r
    if case.model == "cnn":
        assert r["rng"] == N, (r["rng"], N)  # the invariant load_state_dict relies on
    donor, restored = r["states"]["donor", 0], r["states"]["restored", 0]
    want = {"params", "grads", "step_dev"} | set(r["images"]) | ({"vel", "rng"} if case.model == "cnn" else {"m", "v"})
    assert set(donor) == want and set(restored) == want, (sorted(donor), sorted(restored))
    assert float(donor["grads"].abs().max()) == 0.0  # the bucket is clear between steps
    assert compare_states(donor, restored) == []
    rr = r["restored"]
    assert rr["global_step"] == N and rr["steps_taken"] == N and rr["ticket"] == 0.0, rr
    assert rr["rng"] == r["rng"]
    assert rr["clip_factor"] == 1.0  # recomputed before it is read; never carried
    assert rr["clips"] == (dict(case.cfg).get("clipnorm", 0.0), dict(case.cfg).get("clipvalue", 0.0))


@pytest.mark.parametrize("result", IDS, indirect=True)
def test_a_skipped_restoration_is_named(result):
    """Each restoration left out in turn: compare_states names exactly the buffers it owns."""
    case, r = result
    moment = "vel" if case.model == "cnn" else "m"
    want = {"sync_weights": r["images"], "step_dev": ["step_dev"], moment: [moment]}
    if case.model == "cnn":
        want["rng"] = ["rng"]
    assert r["controls"] == want


def _norm(t: torch.Tensor) -> float:
    return float(t.double().norm())


@pytest.mark.parametrize("result", IDS, indirect=True)
def test_continuation_equals_the_uninterrupted_run(result):
    """Steps N + 1 .. N + 3 on the restored engine against the donor that ran straight on. The
    bound is what two uninterrupted runs (donor, twin) differ by: where they agree bit for bit at
    every step, so must the restored run; where fp32 atomics make them differ, the restored run
    may differ from the donor, buffer by buffer, by 3x the donor-twin norm + 1e-6 of the buffer's
    norm (tests/test_step_gpu.py::test_run_many_equals_single_replays' rule). Counters are exact
    either way. Measured (MI355X): every route came out bit-exact except the CNN's GEMM path
    (cnn_b64_gemm: split-K fp32 atomics; donor-twin parameter norm 8e-11 of 5.0, restored 3e-11)."""
    from wellflow.train.state_ref import compare_states

    case, r = result
    S = r["states"]
    exact = all(compare_states(S["donor", j], S["twin", j]) == [] for j in range(MORE + 1))
    noise = max(_norm(S["donor", j]["params"] - S["twin", j]["params"]) for j in range(MORE + 1))
    worst = max(_norm(S["donor", j]["params"] - S["restored", j]["params"]) for j in range(MORE + 1))
    print(f"\nresume[{case.id}] donor-twin {'bit-exact' if exact else 'differ'}: params noise {noise:.3e}, "
          f"restored-donor {worst:.3e}, |params| {_norm(S['donor', MORE]['params']):.3e}")
    assert r["restored_end"] == (r["N"] + MORE, r["N"] + MORE, None if r["rng"] is None else r["N"] + MORE)
    for j in range(1, MORE + 1):
        d, t, s = S["donor", j], S["twin", j], S["restored", j]
        ld, lt, ls = (r["losses"][who, j] for who in ("donor", "twin", "restored"))
        if exact:
            assert compare_states(d, s) == [], (j, compare_states(d, s))
            assert ls == ld, (j, ls, ld)
            continue
        assert compare_states({k: d[k] for k in ("step_dev", "grads")}, {k: s[k] for k in ("step_dev", "grads")}) == []
        for k in d:
            if not d[k].is_floating_point():
                assert torch.equal(d[k], s[k]), (j, k)
                continue
            got, seen = _norm(d[k].float() - s[k].float()), _norm(d[k].float() - t[k].float())
            assert got <= 3.0 * seen + 1e-6 * _norm(d[k]), (j, k, got, seen)
        assert abs(ls - ld) <= 3.0 * abs(lt - ld) + 1e-5 * abs(ld), (j, ls, ld, lt)


# --------------------------------------------------------------------------- the jobs, end to end
NAMES = "well,field,t,whp,choke,glr,temp,water_cut,dsp,flow"
TYPES = "string,string,int,float,float,float,float,float,float,float"
JOBS = {
    "mlp_default": ("mlp", "300", []),
    "mlp_b4096": ("mlp", "4400", ["--batch-size", "4096"]),  # 16,896 training rows: 4 steps per epoch
    "lstm_b64": ("lstm", "300", ["--seq-len", "16", "--hidden", "128", "--batch-size", "64"]),
    "cnn_b20": ("cnn", "300", ["--batch-size", "20"]),
    "cnn_b64_dropout": ("cnn", "300", ["--batch-size", "64", "--dropout", "0.5"]),
}


def _job(model, storage, synth_steps, extra):
    from wellflow.train.job import run_job
    from wellflow.utils import checkpoint

    out = run_job(model, [NAMES, TYPES, "flow", str(storage) + "/", "--synth-wells", "6", "--synth-steps", synth_steps,
                          "--patience", "100", "--verbose", "0", "--device", "cuda", *extra], log=lambda *a, **k: None)
    assert out["native"]
    sd = checkpoint.load_state(str(storage / "models" / f"{model}.ckpt"))
    _, _, mdl = checkpoint.load_mdl(str(storage / "models" / f"{model}.mdl"))
    return {"steps": out["steps"], "epochs": out["epochs"], "loss": list(out["history"]["loss"]),
            "val_loss": list(out["history"]["val_loss"]), "test_loss": out["test_loss"], "params": sd["params"],
            "chunks_done": sd["extra"].get("chunks_done"), "best_epoch": mdl["epoch"]}


def _held_to_measured_noise(tag, A, A2, B):
    """Run B (stopped and resumed) against the uninterrupted run A, within what a second
    uninterrupted run A2 differs from A by: bit for bit where A2 == A, else 3x + 1e-6."""
    scal = lambda r: torch.tensor(r["loss"] + r["val_loss"] + [r["test_loss"]], dtype=torch.float64)  # noqa: E731
    assert B["steps"] == A["steps"] == A2["steps"] and B["epochs"] == A["epochs"] == A2["epochs"], (A, B)
    assert len(B["loss"]) == len(A["loss"]) and len(B["val_loss"]) == len(A["val_loss"])
    exact = torch.equal(scal(A), scal(A2)) and torch.equal(A["params"], A2["params"])
    noise_p, got_p = _norm(A["params"] - A2["params"]), _norm(A["params"] - B["params"])
    noise_s, got_s = (scal(A) - scal(A2)).abs(), (scal(A) - scal(B)).abs()
    print(f"\nresume job[{tag}] A-A' {'bit-exact' if exact else 'differ'}: params noise {noise_p:.3e} resumed {got_p:.3e}"
          f" |params| {_norm(A['params']):.3e}; scalars noise {float(noise_s.max()):.3e} resumed {float(got_s.max()):.3e}")
    if exact:
        assert torch.equal(scal(A), scal(B)) and torch.equal(A["params"], B["params"]), (got_p, got_s)
    else:
        assert got_p <= 3.0 * noise_p + 1e-6 * _norm(A["params"]), (got_p, noise_p)
        assert bool((got_s <= 3.0 * noise_s + 1e-6 * scal(A).abs()).all()), (got_s, noise_s)
    assert B["best_epoch"] == A["best_epoch"], (B["best_epoch"], A["best_epoch"])


@pytest.mark.parametrize("job", list(JOBS))
def test_resumed_job_equals_the_job_run_in_one_go(tmp_path, monkeypatch, job):
    """--epochs 2, then --resume --epochs 4 on the same storage path, against --epochs 4 in one go
    (no --fail-at-step: it switches the K-step launches and the grouped replays off)."""
    monkeypatch.delenv("WELLFLOW_FAIL_AT_STEP", raising=False)
    monkeypatch.delenv("TORCHELASTIC_RESTART_COUNT", raising=False)
    model, synth, extra = JOBS[job]
    for d in "abc":
        (tmp_path / d).mkdir()
    A = _job(model, tmp_path / "a", synth, extra + ["--epochs", "4"])
    A2 = _job(model, tmp_path / "b", synth, extra + ["--epochs", "4"])
    B1 = _job(model, tmp_path / "c", synth, extra + ["--epochs", "2"])
    B = _job(model, tmp_path / "c", synth, extra + ["--epochs", "4", "--resume"])
    assert A["epochs"] == 4 and B1["epochs"] == 2 and A["steps"] == 2 * B1["steps"] >= 8, (A["steps"], B1["steps"])
    assert B["loss"][:2] == B1["loss"] and B["val_loss"][:2] == B1["val_loss"]  # the history came back as saved
    _held_to_measured_noise(job, A, A2, B)


@pytest.mark.parametrize("route,batch", [("staged", 256), ("ring", 320)])
def test_resumed_online_job_equals_the_pass_run_in_one_go(tmp_path, monkeypatch, route, batch):
    """mlp_online, one pass of 4 chunks: stopped by --max-steps on the boundary after chunk 2 and
    resumed, against the pass in one go; through the staged small-batch route (K-step launches on
    whole chunks in device buffers) and the per-batch ring (batch 320: the small kernel refuses)."""
    from wellflow.config import parse_argv
    from wellflow.data.pipeline import prepare
    from wellflow.train import online

    monkeypatch.delenv("WELLFLOW_FAIL_AT_STEP", raising=False)
    monkeypatch.delenv("TORCHELASTIC_RESTART_COUNT", raising=False)
    ran = {"staged": 0, "ring": 0}
    stage_copy, ring_chunk = online._ChunkStage.copy, online._train_chunk_streamed
    monkeypatch.setattr(online._ChunkStage, "copy",
                        lambda self, *a: (ran.__setitem__("staged", ran["staged"] + 1), stage_copy(self, *a))[1])
    monkeypatch.setattr(online, "_train_chunk_streamed",
                        lambda *a: (ran.__setitem__("ring", ran["ring"] + 1), ring_chunk(*a))[1])
    synth = "700"
    base = [NAMES, TYPES, "flow", str(tmp_path) + "/", "--synth-wells", "6", "--synth-steps", synth]
    n = len(prepare(parse_argv("mlp_online", base)).train[0])
    chunk = -(-n // 4)
    starts = online.chunk_bounds(n, chunk, batch)
    assert len(starts) == 4 and all(s % batch == 0 for s in starts), (n, starts)
    extra = ["--batch-size", str(batch), "--online-chunk", str(chunk), "--epochs", "1"]
    for d in "abc":
        (tmp_path / d).mkdir()
    A = _job("mlp_online", tmp_path / "a", synth, extra)
    assert ran[route] > 0 and ran["ring" if route == "staged" else "staged"] == 0, ran
    A2 = _job("mlp_online", tmp_path / "b", synth, extra)
    B1 = _job("mlp_online", tmp_path / "c", synth, extra + ["--max-steps", str(starts[2] // batch)])
    B = _job("mlp_online", tmp_path / "c", synth, extra + ["--resume"])
    assert (A["chunks_done"], B1["chunks_done"], B["chunks_done"]) == (4, 2, 4)
    assert B1["steps"] == starts[2] // batch and len(B1["loss"]) == 2 and len(B["loss"]) == len(A["loss"]) == 4
    assert B["loss"][:2] == B1["loss"] and B["val_loss"][:2] == B1["val_loss"]
    _held_to_measured_noise(f"mlp_online {route}", A, A2, B)
