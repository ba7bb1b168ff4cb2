"""Gradient clipping of the flat optimizers (Keras 0.x ``clipnorm`` / ``clipvalue``) on the CPU:
the rule itself, FlatAdam against float64 and torch's own clipping, state dicts, the job flags,
one end-to-end job step and one data-parallel step over gloo."""
import json
import os
import socket
import subprocess
import sys
import textwrap

import pytest
import torch

from wellflow.config import parse_argv
from wellflow.optim.flat import FlatAdam, FlatSGD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = "well,field,t,whp,choke,glr,temp,water_cut,dsp,flow"
TYPES = "string,string,int,float,float,float,float,float,float,float"


def _plain_sgd(n=37, lr=0.5, seed=0, **kw):
    g = torch.Generator().manual_seed(seed)
    p, gr = torch.randn(n, generator=g), torch.randn(n, generator=g)
    p0 = p.clone()
    return p0, p, gr, FlatSGD(p, gr, lr=lr, momentum=0.0, nesterov=False, decay=0.0, **kw)


def test_clipnorm_scales_to_c_only_at_or_above_c():
    p0, p, g, opt = _plain_sgd(clipnorm=1.0)
    n = g.norm().item()
    assert n > 1.0
    opt.step()
    torch.testing.assert_close(p0 - p, 0.5 * g * (1.0 / n), rtol=1e-5, atol=1e-7)
    torch.testing.assert_close((p0 - p).norm(), torch.tensor(0.5), rtol=1e-5, atol=0)
    # below the bound nothing changes: the move is lr * g
    p0, p, g, opt = _plain_sgd(clipnorm=100.0)
    assert g.norm().item() < 100.0
    opt.step()
    assert torch.equal(p, p0 - 0.5 * g)
    assert opt.clip_stats()["clipped_steps"] == 0


def test_clipvalue_clamps_each_element():
    p0, p, g, opt = _plain_sgd(clipvalue=0.3)
    assert (g.abs() > 0.3).any() and (g.abs() < 0.3).any()
    opt.step()
    assert torch.equal(p, p0 - 0.5 * g.clamp(-0.3, 0.3))


def test_norm_scaling_comes_before_the_clamp():
    p0, p, g, opt = _plain_sgd(clipnorm=1.0, clipvalue=0.2)
    scaled = g * (1.0 / g.norm().item())
    assert (scaled.abs() > 0.2).any()
    assert not torch.equal(scaled.clamp(-0.2, 0.2), (g.clamp(-0.2, 0.2)) * (1.0 / g.clamp(-0.2, 0.2).norm().item()))
    opt.step()
    torch.testing.assert_close(p0 - p, 0.5 * scaled.clamp(-0.2, 0.2), rtol=1e-5, atol=1e-7)


def test_grad_scale_counts_in_the_norm():
    # ||g|| > 1 but ||g * grad_scale|| < 1: no clipping; and the other way round
    p0, p, g, opt = _plain_sgd(clipnorm=1.0)
    s = 0.5 / g.norm().item()
    opt.step(grad_scale=s)
    assert torch.equal(p, p0 - 0.5 * (g * s))
    assert opt.clip_stats()["clipped_steps"] == 0
    torch.testing.assert_close(torch.tensor(opt.clip_stats()["grad_norm_last"]), torch.tensor(0.5), rtol=1e-5, atol=0)
    p0, p, g, opt = _plain_sgd(clipnorm=1.0)
    s = 4.0 / g.norm().item()
    opt.step(grad_scale=s)
    torch.testing.assert_close((p0 - p).norm(), torch.tensor(0.5), rtol=1e-5, atol=0)
    assert opt.clip_stats()["clipped_steps"] == 1


def test_non_finite_norm_leaves_the_gradient_unscaled():
    p0, p, g, opt = _plain_sgd(clipnorm=1.0)
    g[3] = float("inf")
    opt.step()
    ok = torch.ones_like(g, dtype=torch.bool)
    ok[3] = False
    assert torch.equal(p[ok], (p0 - 0.5 * g)[ok])
    st = opt.clip_stats()
    assert st["clipped_steps"] == 0 and st["grad_norm_last"] == float("inf") and st["grad_norm_max"] == float("inf")


def _adam_f64(p, grads, lr, b1, b2, eps, clipnorm, clipvalue):
    """Adam with PyTorch's bias corrections on the Keras-clipped gradient, in float64."""
    p = p.double().clone()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    for t, g in enumerate(grads, 1):
        g = g.double()
        n = g.norm().item()
        if clipnorm > 0 and n >= clipnorm:
            g = g * (clipnorm / n)
        if clipvalue > 0:
            g = g.clamp(-clipvalue, clipvalue)
        m = b1 * m + (1 - b1) * g
        v = b2 * v + (1 - b2) * g * g
        p = p - lr * (m / (1 - b1**t)) / ((v / (1 - b2**t)).sqrt() + eps)
    return p, m, v


@pytest.mark.parametrize("clipvalue", [0.0, 0.05])
def test_adam_three_steps_against_float64_and_torch(clipvalue):
    """Gradient magnitudes 10, 0.01 and 1 against clipnorm 1: steps 1 and 3 clip, step 2 does not.
    After ONE Adam step the update is +-lr whatever the scale, so the moments and several steps
    are compared, not the first step's parameters alone."""
    gen = torch.Generator().manual_seed(1)
    n, lr, c = 53, 1e-2, 1.0
    p0 = torch.randn(n, generator=gen)
    grads = [torch.randn(n, generator=gen) * s for s in (10.0, 0.01, 1.0)]
    norms = [g.norm().item() for g in grads]
    assert norms[0] > c and norms[1] < c and norms[2] > c
    p, gr = p0.clone(), torch.zeros(n)
    opt = FlatAdam(p, gr, lr=lr, clipnorm=c, clipvalue=clipvalue)
    # torch.optim.Adam + torch.nn.utils (max_norm's 1e-6 in the denominator is below fp32 here)
    tp = torch.nn.Parameter(p0.clone())
    topt = torch.optim.Adam([tp], lr=lr)
    for g in grads:
        gr.copy_(g)
        opt.step()
        tp.grad = g.clone()
        torch.nn.utils.clip_grad_norm_([tp], c)
        if clipvalue:
            torch.nn.utils.clip_grad_value_([tp], clipvalue)
        topt.step()
    rp, rm, rv = _adam_f64(p0, grads, lr, 0.9, 0.999, 1e-8, c, clipvalue)
    torch.testing.assert_close(opt.m.double(), rm, rtol=1e-5, atol=1e-9)
    torch.testing.assert_close(opt.v.double(), rv, rtol=1e-5, atol=1e-12)
    torch.testing.assert_close(p.double(), rp, rtol=1e-5, atol=1e-6)
    st = topt.state[tp]
    torch.testing.assert_close(opt.m, st["exp_avg"], rtol=1e-5, atol=1e-9)
    torch.testing.assert_close(opt.v, st["exp_avg_sq"], rtol=1e-5, atol=1e-12)
    torch.testing.assert_close(p, tp.detach(), rtol=1e-5, atol=1e-6)
    # the clipping mattered: the unclipped moments are far away
    _, um, _ = _adam_f64(p0, grads, lr, 0.9, 0.999, 1e-8, 0.0, 0.0)
    assert (um - rm).abs().max().item() > 0.1
    stats = opt.clip_stats()
    assert stats["clipped_steps"] == 2
    assert stats["grad_norm_last"] == pytest.approx(norms[2], rel=1e-5)
    assert stats["grad_norm_max"] == pytest.approx(norms[0], rel=1e-5)


@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_state_dict_round_trip_and_older_checkpoints(kind, tmp_path):
    cls = FlatAdam if kind == "adam" else FlatSGD
    p, g = torch.randn(9), torch.randn(9)
    opt = cls(p, g, clipnorm=0.5, clipvalue=0.1)
    opt.step()
    sd = opt.state_dict()
    assert sd["clipnorm"] == 0.5 and sd["clipvalue"] == 0.1
    path = tmp_path / "opt.ckpt"
    torch.save(sd, path)
    sd = torch.load(path, weights_only=True)
    other = cls(p.clone(), g.clone())
    assert not other.clips
    other.load_state_dict(sd)
    assert other.clipnorm == 0.5 and other.clipvalue == 0.1 and other.clips
    # a state dict from before the two settings existed
    old = {k: v for k, v in sd.items() if k not in ("clipnorm", "clipvalue")}
    other.load_state_dict(old)
    assert other.clipnorm == 0.0 and other.clipvalue == 0.0 and not other.clips


def test_clip_stats_count_and_reset():
    p, g = torch.zeros(4), torch.zeros(4)
    opt = FlatSGD(p, g, lr=0.1, momentum=0.0, nesterov=False, decay=0.0, clipnorm=1.0)
    for s in (3.0, 0.1, 5.0, 0.2):
        g.copy_(torch.tensor([s, 0.0, 0.0, 0.0]))
        opt.step()
    st = opt.clip_stats(reset=True)
    assert st == {"grad_norm_last": pytest.approx(0.2), "grad_norm_max": pytest.approx(5.0), "clipped_steps": 2}
    assert opt.clip_stats() == {"grad_norm_last": 0.0, "grad_norm_max": 0.0, "clipped_steps": 0}
    # off by default
    assert not FlatSGD(p, g).clips and not FlatAdam(p, g).clips


def test_argv_sets_the_fields():
    cfg = parse_argv("lstm", [NAMES, TYPES, "flow", "/tmp/x", "--clipnorm", "0.5", "--clipvalue", "0.1"])
    assert cfg.clipnorm == 0.5 and cfg.clipvalue == 0.1
    assert cfg.clip == 6.0  # the mae_clip loss bound is another setting
    cfg = parse_argv("cnn", [NAMES, TYPES, "flow", "/tmp/x"])
    assert cfg.clipnorm == 0.0 and cfg.clipvalue == 0.0


def _mdl_flat(path):
    from wellflow.utils import checkpoint as ckpt

    _, layers, _ = ckpt.load_mdl(str(path))
    return torch.cat([p.reshape(-1).double() for _, params in layers for p in params])


def test_cpu_mlp_job_first_step_moves_by_lr_times_c(tmp_path):
    """One SGD step (no momentum, no decay) of the MLP job with clipnorm c far below the first
    gradient's norm: ||delta params|| = lr * c. The start point is the same job at lr 0."""
    from wellflow.train.job import run_job

    lr, c = 1.0, 0.05
    flat = {}
    for name, rate in (("start", 0.0), ("moved", lr)):
        store = tmp_path / name
        metrics = tmp_path / f"{name}.jsonl"
        run_job("mlp", [NAMES, TYPES, "flow", str(store), "--epochs", "1", "--synth-wells", "3", "--synth-steps", "120",
                        "--batch-size", "64", "--mlp-hidden", "16,8", "--device", "cpu", "--precision", "fp32",
                        "--optimizer", "sgd", "--momentum", "0", "--no-nesterov", "--decay", "0", "--lr", str(rate),
                        "--clipnorm", str(c), "--max-steps", "1", "--metrics", str(metrics)],
                log=lambda *a, **k: None)
        flat[name] = _mdl_flat(store / "models" / "mlp.mdl")
        rec = json.loads(open(metrics).read().splitlines()[-1])
        assert rec["global_step"] == 1 and rec["clipped_steps"] == 1
        assert rec["grad_norm_last"] > 10 * c, rec  # c is far below the gradient's norm
        assert rec["grad_norm_max"] == rec["grad_norm_last"]
    moved = (flat["moved"] - flat["start"]).norm().item()
    assert moved == pytest.approx(lr * c, rel=1e-5)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _torchrun(tmp_path, body: str, nproc: int, timeout=300):
    """tests/test_dist_gloo.py's harness: ``body`` on ``nproc`` gloo ranks, one JSON per rank."""
    script = tmp_path / "worker.py"
    script.write_text(textwrap.dedent(f"""
        import json, os, sys
        sys.path.insert(0, {ROOT!r})
        import torch
        from wellflow.parallel.dist import DistContext
        OUT = {str(tmp_path)!r}
    """) + textwrap.dedent(body))
    env = dict(os.environ)
    env["CUDA_VISIBLE_DEVICES"] = ""
    env["OMP_NUM_THREADS"] = "1"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}",
           "--max-restarts=0", "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), str(script)]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=timeout, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return [json.load(open(tmp_path / f"rank{i}.json")) for i in range(nproc)]


def test_dp_clipped_step_equals_single_process_clipped_step(tmp_path):
    """World 2 over gloo: a clipped step on two half batches == the clipped single-process step on
    the whole batch, i.e. the norm is that of the all-reduced gradient. Clipping each rank's half
    gradient before the reduction would give another result (``pre``)."""
    res = _torchrun(tmp_path, """
        from wellflow.models.base import TorchEngine
        from wellflow.models.mlp import MLPRegressor
        from wellflow.optim.flat import FlatSGD
        from wellflow.train.step import StepRunner
        N, C = 32, 0.05
        g = torch.Generator().manual_seed(0)
        X, Y = torch.randn(N, 6, generator=g), torch.randn(N, generator=g) * 3
        ctx = DistContext.from_env(device="cpu")
        W, r = ctx.world_size, ctx.rank
        B = N // W
        def sgd(eng):
            return FlatSGD(eng.params, eng.grads, lr=0.5, momentum=0.9, zero_grads=True, clipnorm=C)
        torch.manual_seed(100)
        eng = TorchEngine(MLPRegressor(6, (16, 8)), loss="mse")
        opt = sgd(eng)
        run = StepRunner(eng, opt, ctx, 1.0 / N, lambda k: (X[r * B:(r + 1) * B], Y[r * B:(r + 1) * B]), graph=False)
        for s in range(3):
            run.run(s)
        torch.manual_seed(100)
        ref = TorchEngine(MLPRegressor(6, (16, 8)), loss="mse")
        ropt = sgd(ref)
        rrun = StepRunner(ref, ropt, DistContext(device=torch.device("cpu")), 1.0 / N, lambda k: (X, Y), graph=False)
        for s in range(3):
            rrun.run(s)
        # what clipping before the reduction would have done on the first step
        torch.manual_seed(100)
        pre = TorchEngine(MLPRegressor(6, (16, 8)), loss="mse")
        p0 = pre.params.clone()
        halves = []
        for q in range(W):
            pre.forward_backward(X[q * B:(q + 1) * B], Y[q * B:(q + 1) * B], grad_scale=1.0 / N)
            h = pre.grads.clone()
            halves.append(h * min(1.0, C / h.norm().item()))
        first = 0.5 * sum(halves)
        ref1 = TorchEngine(MLPRegressor(6, (16, 8)), loss="mse")
        ref1.params.copy_(p0)
        ref1.forward_backward(X, Y, grad_scale=1.0 / N)
        full = ref1.grads.clone()
        post = 0.5 * full * min(1.0, C / full.norm().item())
        json.dump({"err": (eng.params - ref.params).abs().max().item(), "p0": eng.params[:5].tolist(),
                   "stats": opt.clip_stats(), "rstats": ropt.clip_stats(),
                   "pre_vs_post": ((first - post).norm() / post.norm()).item()},
                  open(f"{OUT}/rank{r}.json", "w"))
        ctx.shutdown()
    """, 2)
    for rr in res:
        assert rr["err"] < 1e-5, rr
        assert rr["stats"]["clipped_steps"] == 3 and rr["rstats"]["clipped_steps"] == 3, rr
        assert rr["stats"]["grad_norm_max"] == pytest.approx(rr["rstats"]["grad_norm_max"], rel=1e-5)
        assert rr["pre_vs_post"] > 1e-3, rr  # the two orders differ on this data, so err separates them
    assert res[0]["p0"] == res[1]["p0"]
