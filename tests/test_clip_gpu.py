"""Gradient clipping on the MI355X: the norm kernel (csrc/elementwise.hip grad_clip_scale_kernel)
against float64, and the four fused update kernels with the clip arguments — adam_dev (MLP:
shadow + transposed block), lstm_adam_pack, sgd_dev and cnn_sgd_pack — against the composition
they replace, inactive clipping bit for bit against no clipping, the captured step against the
eager one, and the job."""
import json
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAMES = "well,field,t,whp,choke,glr,temp,water_cut,dsp,flow"
TYPES = "string,string,int,float,float,float,float,float,float,float"


# ------------------------------------------------------------------------------ the norm kernel
def _chain(n: int) -> int:
    """k of csrc/elementwise.hip grad_clip_scale_kernel: the longest chain of fp32 additions an
    element passes through, from the launcher's constants (256 threads, <= 256 workgroups)."""
    n4 = n // 4
    grid = min(256, max(1, min(2048, (n4 + 255) // 256)))
    iters = -(-n4 // (grid * 256))
    return iters + 11


def _clip_buffers():
    state = torch.zeros(8, device=DEV)
    state[0] = 1.0
    return torch.zeros(256, device=DEV), state


def _launch(g, c, gscale=1.0, bufs=None):
    from wellflow.ops.native import lib

    partial, state = bufs or _clip_buffers()
    lib().grad_clip_scale(g, gscale, c, partial, state)
    torch.cuda.synchronize()
    assert int(state.view(torch.int32)[4].item()) == 0, "the ticket was not reset"
    return state


def _within_one_ulp(x: float, ref: torch.Tensor) -> bool:
    lo = torch.nextafter(ref, torch.tensor(-math.inf))
    hi = torch.nextafter(ref, torch.tensor(math.inf))
    return lo.item() <= x <= hi.item()


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 1024, 65536 + 3, 2**20 + 5, "view"])
def test_norm_kernel_against_float64(n):
    gen = torch.Generator(device=DEV).manual_seed(11)
    if n == "view":  # a length that is no multiple of 4 inside a larger buffer: nothing past it is read
        buf = torch.full((5000,), 1e10, device=DEV)
        g = buf[:4098]
        g.copy_(torch.randn(4098, device=DEV, generator=gen))
        n = 4098
    else:
        g = torch.randn(n, device=DEV, generator=gen) + (0.5 if n == 1 else 0.0)
    gscale = 0.25
    ref = (g.double().cpu() * gscale).pow(2).sum().sqrt().item()
    c = 0.5 * ref
    a = _launch(g, c, gscale).cpu()
    k = _chain(n)
    assert n < 2**20 or k > 12  # the grid-stride loop runs more than once at the largest size
    rel = abs(a[1].item() - ref) / ref
    print(f"n={n} k={k} rel={rel:.3e} bound={k * 2.0**-23:.3e}")
    assert rel <= k * 2.0**-23, (n, rel, k)
    assert _within_one_ulp(a[0].item(), torch.tensor(c, dtype=torch.float32) / a[1]), a
    assert a[2].item() == 1.0 and a[3].item() == a[1].item()
    # below the bound: factor exactly 1, nothing counted
    b = _launch(g, 2.0 * ref, gscale).cpu()
    assert b[0].item() == 1.0 and b[2].item() == 0.0 and b[1].item() == a[1].item()
    # order independence: a second launch on the same data gives the same bits
    a2 = _launch(g, c, gscale).cpu()
    assert torch.equal(a.view(torch.int32), a2.view(torch.int32))


def test_norm_kernel_zero_and_inf_buckets():
    z = _launch(torch.zeros(70001, device=DEV), 1.0).cpu()
    assert z[0].item() == 1.0 and z[1].item() == 0.0 and z[2].item() == 0.0 and not torch.isnan(z).any()
    g = torch.randn(70001, device=DEV)
    g[69999] = float("inf")
    s = _launch(g, 1.0).cpu()
    assert s[0].item() == 1.0 and s[1].item() == math.inf and s[2].item() == 0.0 and s[3].item() == math.inf


def test_norm_kernel_statistics_accumulate_on_the_device():
    bufs = _clip_buffers()
    g = torch.zeros(1000, device=DEV)
    for v in (3.0, 0.5, 7.0, 0.25):
        g.zero_()
        g[17] = v
        st = _launch(g, 1.0, bufs=bufs)
    st = st.cpu()
    assert st[1].item() == 0.25 and st[2].item() == 2.0 and st[3].item() == 7.0 and st[0].item() == 1.0


# ------------------------------------------------------------------- the four update kernels
KINDS = ["lstm_f16", "lstm_f100", "cnn_pack", "cnn_plain", "mlp_f16", "mlp_f18"]


def _make(kind, **clip):
    """(engine, optimizer, names of the optimizer's moment tensors, names of the bf16 images):
    lstm_* -> lstm_adam_pack_kernel, cnn_pack -> cnn_sgd_pack_kernel, cnn_plain -> sgd_dev_kernel,
    mlp_* -> adam_dev_kernel with the shadow and the transposed W2 block."""
    from wellflow.optim.flat import FlatAdam, FlatSGD

    if kind.startswith("lstm"):
        from wellflow.models.lstm import NativeLSTM, init_lstm_flat

        F = 16 if kind == "lstm_f16" else 100  # KX = 32 / 128
        eng = NativeLSTM(F, 512, 8, 512, device=DEV)
        eng.params.copy_(init_lstm_flat(F, 512, seed=2).to(DEV))
        eng.sync_weights()
        opt = FlatAdam(eng.params, eng.grads, lr=1e-3, zero_grads=True, writeback=eng, **clip)
        assert eng.fused_adam_ok(opt)
        return eng, opt, ("m", "v"), ("Wp", "WhhT")
    if kind.startswith("cnn"):
        from wellflow.models.cnn import CNN1DRegressor, NativeCNN

        ref = CNN1DRegressor(dropout=0.5).init_keras(5)
        eng = NativeCNN(ref.layout, batch=512, device=DEV, dropout=0.5, loss="mae_clip", seed=3)
        eng.params.copy_(ref.to_flat().to(DEV))
        eng.sync_weights()
        opt = FlatSGD(eng.params, eng.grads, lr=0.01, zero_grads=True, writeback=eng if kind == "cnn_pack" else None, **clip)
        assert eng.fused_sgd_ok(opt)
        return eng, opt, ("vel",), ("WcA", "WdF", "WdB")
    from wellflow.models.mlp import NativeMLP, init_mlp_flat

    F = 16 if kind == "mlp_f16" else 18  # Fp = 16 / 24
    eng = NativeMLP(F, (256, 256), 256, device=DEV)
    eng.params.copy_(init_mlp_flat(F, (256, 256), seed=5).to(DEV))
    eng.sync_weights()
    opt = FlatAdam(eng.params, eng.grads, lr=1e-3, shadow=eng.shadow, zero_grads=True, shadow_t=eng.shadow_t, **clip)
    return eng, opt, ("m", "v"), ("shadow", "w2t") if eng.w2t is not None else ("shadow",)


def _after(eng, opt):
    if opt.writeback is None and getattr(opt, "shadow", None) is None:
        eng.sync_weights()


def _images_are_a_repack(eng, images):
    got = {nm: getattr(eng, nm).clone() for nm in images}
    eng.sync_weights()
    torch.cuda.synchronize()
    for nm, t in got.items():
        assert torch.equal(t, getattr(eng, nm)), nm


@pytest.mark.parametrize("kind", KINDS)
def test_inactive_clip_is_free(kind):
    """clipnorm above every norm: the factor is exactly 1.0f, and three steps leave every tensor
    bit-identical to clipnorm = 0 (which launches nothing extra and hands the kernels no state)."""
    a, oa, moments, images = _make(kind, clipnorm=1e30)
    b, ob, _, _ = _make(kind)
    assert ob.clip_args(0.5) == (None, 0.0)
    gen = torch.Generator(device=DEV).manual_seed(5)
    for _ in range(3):
        gr = torch.randn(a.grads.shape, device=DEV, generator=gen) * 1e-2
        for eng, opt in ((a, oa), (b, ob)):
            eng.grads.copy_(gr)
            opt.step(0.5)
            _after(eng, opt)
    torch.cuda.synchronize()
    assert oa.clip_state[0].item() == 1.0 and oa.clip_stats()["clipped_steps"] == 0
    assert oa.clip_stats()["grad_norm_last"] > 0.0
    assert torch.equal(a.params, b.params) and torch.equal(oa.step_dev, ob.step_dev)
    for nm in moments:
        assert torch.equal(getattr(oa, nm), getattr(ob, nm)), nm
    for nm in images:
        assert torch.equal(getattr(a, nm), getattr(b, nm)), nm


@pytest.mark.parametrize("both", [False, True], ids=["norm", "norm+value"])
@pytest.mark.parametrize("kind", KINDS)
def test_active_clip_equals_scale_then_update(kind, both):
    """Three steps on given gradients of magnitude 10 c, c / 10 and 10 c (steps 1 and 3 clip):
    the fused clipped update == the bucket multiplied by the device's factor (and clamped) with
    torch ops, then the same optimizer with clipping off."""
    c, gscale = 1.0, 0.5
    b, ob, moments, images = _make(kind)
    n = b.params.numel()
    per = c / (gscale * math.sqrt(n))  # the element size at which ||gscale g|| = c
    v = c / math.sqrt(n) if both else 0.0  # one sigma of a clipped step's elements
    a, oa, _, _ = _make(kind, clipnorm=c, clipvalue=v)
    gen = torch.Generator(device=DEV).manual_seed(6)
    factors, clamped = [], 0
    for s in (10.0, 0.1, 10.0):
        gr = torch.randn(a.grads.shape, device=DEV, generator=gen) * (s * per)
        a.grads.copy_(gr)
        oa.step(gscale)
        _after(a, oa)
        f = oa.clip_state[0].clone()
        factors.append(f)
        eff = gr * (torch.tensor(gscale, device=DEV) * f)  # fp32, as the kernels form g * gs
        if both:
            clamped += int((eff.abs() > v).sum().item())
            eff = eff.clamp(-v, v)
        b.grads.copy_(eff)
        ob.step(1.0)
        _after(b, ob)
    torch.cuda.synchronize()
    fs = [f.item() for f in factors]
    assert fs[0] < 0.2 and fs[1] == 1.0 and fs[2] < 0.2, fs
    assert oa.clip_stats()["clipped_steps"] == 2
    assert not both or clamped > n // 10
    torch.testing.assert_close(a.params, b.params, rtol=1e-5, atol=1e-8)
    for nm in moments:
        torch.testing.assert_close(getattr(oa, nm), getattr(ob, nm), rtol=1e-5, atol=1e-8)
    assert torch.equal(oa.step_dev, ob.step_dev)
    _images_are_a_repack(a, images)
    assert a.grads.abs().max().item() == 0.0  # the bucket was cleared


def test_clipvalue_alone_launches_no_norm_kernel():
    """clipvalue without clipnorm: the update gets no state block, only the clamp."""
    from wellflow.optim.flat import FlatSGD

    n = 1003
    p, g = torch.zeros(n, device=DEV), torch.randn(n, device=DEV)
    g0 = g.clone()
    opt = FlatSGD(p, g, lr=1.0, momentum=0.0, nesterov=False, decay=0.0, clipvalue=0.3)
    assert opt.clip_args(1.0) == (None, 0.3)
    opt.step()
    torch.cuda.synchronize()
    assert torch.equal(p, -(g0.clamp(-0.3, 0.3)))
    assert opt.clip_stats() == {"grad_norm_last": 0.0, "grad_norm_max": 0.0, "clipped_steps": 0}


# ----------------------------------------------------------------------------------- the graph
def _step_engine(model):
    """The shapes of tests/test_step_gpu.py."""
    if model == "lstm":
        from wellflow.data.synth import synth_lstm_batch
        from wellflow.models.lstm import NativeLSTM, init_lstm_flat

        B, T, F, H = 2048, 16, 16, 512
        eng = NativeLSTM(F, H, T, B, device=DEV)
        eng.params.copy_(init_lstm_flat(F, H, seed=3).to(DEV))
        x, y = synth_lstm_batch(B, T, F, seed=3)
    else:
        from wellflow.data.synth import synth_tabular_batch
        from wellflow.models.mlp import NativeMLP, init_mlp_flat

        B, F = 65536, 16
        eng = NativeMLP(F, (256, 256), B, device=DEV)
        eng.params.copy_(init_mlp_flat(F, (256, 256), seed=2).to(DEV))
        x, y = synth_tabular_batch(B, F, seed=2)
    eng.sync_weights()
    return eng, x.to(DEV), y.to(DEV)


# targets scaled per step: x 1 gives the data's own gradient norm (1.5 - 4 on both models at
# these shapes), x 100 one of 200 - 1100. GRAPH_CLIP lies between the two, a factor 3 or more from
# either (the test checks it), so steps 1, 4 and 6 clip: the capture (step 3) does not, two of the
# three replays do.
Y_SCALE = (100.0, 1.0, 1.0, 100.0, 1.0, 100.0)
GRAPH_CLIP = 20.0


@pytest.mark.parametrize("model", ["lstm", "mlp"])
def test_step_graph_with_clipping_equals_eager(model):
    """StepRunner(graph=True) with a clipping optimizer, 6 steps (2 eager, capture, 3 replays),
    against 6 eager steps: parameters within the graph-vs-eager bound of tests/test_step_gpu.py,
    and the same number of clipped steps, so a replay recomputes the norm (a factor baked in at
    the capture, an unclipped step, would clip none of the replays)."""
    from wellflow.optim.flat import FlatAdam
    from wellflow.parallel.dist import DistContext
    from wellflow.train.step import StepRunner

    clip = GRAPH_CLIP
    eng_e, x, y = _step_engine(model)
    y0 = y.clone()
    opt_e = FlatAdam(eng_e.params, eng_e.grads, lr=1e-3, clipnorm=clip)
    norms = []
    for s in Y_SCALE:
        y.copy_(y0 * s)
        eng_e.forward_backward(x, y, 1.0 / len(y), zero_grads=True)
        opt_e.step()
        eng_e.sync_weights()
        norms.append(opt_e.clip_state[1].item())
    print(f"{model}: eager gradient norms {norms}, clipnorm {clip}")
    # the bound is far from every step's norm: summation-order noise cannot flip a decision
    for nrm, s in zip(norms, Y_SCALE):
        assert nrm > 3 * clip if s > 1 else nrm < clip / 3, (norms, clip)
    stats_e = opt_e.clip_stats()
    assert stats_e["clipped_steps"] == 3

    eng_g, xg, yg = _step_engine(model)
    kw = {"shadow": eng_g.shadow} if hasattr(eng_g, "shadow") else {"writeback": eng_g}
    opt_g = FlatAdam(eng_g.params, eng_g.grads, lr=1e-3, zero_grads=True, clipnorm=clip, **kw)
    run = StepRunner(eng_g, opt_g, DistContext(device=torch.device(DEV)), 1.0 / len(yg), lambda k: (xg, yg), graph=True)
    for s in Y_SCALE:
        yg.copy_(y0 * s)
        run.run()
    torch.cuda.synchronize()
    assert run.graphs, "the step was never captured"
    assert opt_g.steps_taken == len(Y_SCALE)
    d = (eng_e.params - eng_g.params).abs().max().item()
    assert d <= 5e-5, d
    stats_g = opt_g.clip_stats()
    assert stats_g["clipped_steps"] == stats_e["clipped_steps"], (stats_g, stats_e)
    assert stats_g["grad_norm_max"] == pytest.approx(stats_e["grad_norm_max"], rel=1e-3)
    assert stats_g["grad_norm_last"] == pytest.approx(stats_e["grad_norm_last"], rel=1e-3)


# ------------------------------------------------------------------------------------- the job
def test_clipping_job_takes_the_regular_path_and_reports_norms(tmp_path, monkeypatch, capfd):
    """The MLP job at its default batch (256): with --clipnorm it leaves the K-steps-per-launch
    path (whose update never sees the whole gradient), says so once, trains with finite loss and
    writes the three clip fields per epoch; without --clipnorm it stays on the K-step path."""
    from wellflow.models import base
    from wellflow.models.mlp import NativeMLP
    from wellflow.train.job import run_job

    monkeypatch.setattr(base, "_NOTED", set())
    fused, reasons = [], []
    real_fused, real_reason = NativeMLP.fused_steps, NativeMLP.small_steps_reason

    def spy_fused(self, *a, **k):
        fused.append(1)
        return real_fused(self, *a, **k)

    def spy_reason(self, *a, **k):
        why = real_reason(self, *a, **k)
        reasons.append(why)
        return why

    monkeypatch.setattr(NativeMLP, "fused_steps", spy_fused)
    monkeypatch.setattr(NativeMLP, "small_steps_reason", spy_reason)

    def job(sub, *extra):
        metrics = tmp_path / f"{sub}.jsonl"
        out = run_job("mlp", [NAMES, TYPES, "flow", str(tmp_path / sub), "--synth-wells", "4", "--synth-steps", "200",
                              "--max-steps", "40", "--device", "cuda", "--metrics", str(metrics), *extra],
                      log=lambda *a, **k: None)
        return out, [json.loads(l) for l in open(metrics)]

    capfd.readouterr()
    out, recs = job("clipped", "--clipnorm", "0.5")
    err = capfd.readouterr().err
    assert out["native"] is True and out["steps"] == 40
    assert not fused and reasons and all(r == base.CLIP_STEPS_REASON for r in reasons)
    assert err.count(base.CLIP_STEPS_REASON) == 1, err
    assert all(math.isfinite(v) for v in out["history"]["loss"]) and math.isfinite(out["test_loss"])
    assert recs
    for rec in recs:
        assert {"grad_norm_last", "grad_norm_max", "clipped_steps"} <= set(rec)
        assert 0.0 < rec["grad_norm_last"] <= rec["grad_norm_max"] < math.inf
        assert isinstance(rec["clipped_steps"], int)
    assert sum(rec["clipped_steps"] for rec in recs) <= 40

    reasons.clear()
    out, recs = job("plain")
    assert fused and reasons and all(r is None for r in reasons)
    assert out["steps"] == 40 and "grad_norm_last" not in recs[0]
    assert base.CLIP_STEPS_REASON not in capfd.readouterr().err
