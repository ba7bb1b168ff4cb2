"""The fused training forward for 65-512 features (csrc/mlp_wide.hip mlp2_fwd_wide_train_kernel) and the
step built on it (NativeMLP._step_wide): float64 bit for bit on exact data (wellflow/train/exact.py)."""
import os
import re
import subprocess
import sys

import pytest
import torch

from wellflow.models.mlp import MlpLayout, NativeMLP
from wellflow.train import exact as ex

pytestmark = pytest.mark.gpu
DEV = "cuda"
HID = (256, 256)
NAN = float("nan")
LOSSES = ("mse", "mae_clip")
_ENG = {}


def _engine(F, loss, flat, batch=300):
    if (F, batch) not in _ENG:
        _ENG[F, batch] = NativeMLP(F, HID, batch, device=DEV, clip=ex.CLIP)
    eng = _ENG[F, batch]
    eng.loss_kind = loss
    eng.params.copy_(flat.float().to(DEV))
    eng.sync_weights()
    return eng


def _case(F, B, loss, idx=None):
    """(case, targets, float64 step), proven exact; ``idx``: the 300-row case's rows repeated to B rows."""
    case = ex.exact_mlp_case(F, HID, B if idx is None else 300, 100 * F + (B if idx is None else 300) + 2)
    if idx is not None:
        case = ex.ExactCase(case.lay, case.flat, case.x[idx], case.e[idx], ex.exact_grad_scale(B))
    y = ex.exact_targets(case)
    assert ex.exactness_violations(case, y, loss) == []
    return case, y, ex.mlp_step_fp64(case.flat, case.x, y, case.grad_scale, loss)


def _blocks(lay, flat):
    layers, hw, hb = lay.views(flat)
    return [layers[0][0], layers[0][1], layers[1][0], layers[1][1], hw, hb]


def _step(eng, x, y, gs, wide=True, **kw):
    for t in (eng.pred, eng.dy, *eng.Hs):
        t.fill_(NAN)
    eng.wide_step = wide
    try:
        return eng.forward_backward(x.to(DEV), y.float().to(DEV), gs, **kw)
    finally:
        eng.wide_step = True


def _check(eng, ref, ls, B, tag, mult=1.0, loss_want=None):
    F = ref["H"][0].shape[1]
    assert torch.equal(eng.pred[:B].cpu(), ref["pred"].float()) and torch.equal(eng.dy[:B].cpu(), ref["dy"].float()), tag
    assert float(ls) == float(ref["loss_sum"] if loss_want is None else loss_want), tag
    assert torch.equal(eng.Hs[0][: B * 256].float().cpu().view(B, 256), ref["H"][1].float()), tag
    for i, (g, w) in enumerate(zip(_blocks(eng.lay, eng.grads.cpu()), _blocks(eng.lay, (mult * ref["grads"]).float()))):
        assert torch.equal(g, w), f"{tag}: gradient block {i}"
    assert not _blocks(eng.lay, eng.grads.cpu())[0][:, F:].any(), f"{tag}: gW1 padding"
    assert eng.pred[B:].isnan().all() and eng.dy[B:].isnan().all() and eng.Hs[0][B * 256:].isnan().all(), tag
    assert eng.Hs[1].isnan().all(), f"{tag}: H2 reached HBM on the fused route"


@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("F", (65, 72, 100, 128, 136, 264, 512))
def test_wide_step_exact(F, loss):
    # F = 72, 512 also at 128 CUs + 1 rows (the 300 exact rows repeated): a workgroup's second tile, its sums carried in LDS
    big = (128 * torch.cuda.get_device_properties(0).multi_processor_count + 1,) if F in (72, 512) else ()
    for B in (1, 64, 127, 128, 129, 300) + big:
        case, y, ref = _case(F, B, loss, idx=torch.arange(B) % 300 if B > 300 else None)
        eng = _engine(F, loss, case.flat, batch=max(300, B))
        _check(eng, ref, _step(eng, case.x.float(), y, case.grad_scale), B, f"F={F} B={B} {loss}")
        wide = eng.grads.clone()
        _step(eng, case.x.float(), y, case.grad_scale, wide=False)
        assert torch.equal(eng.grads, wide) and not eng.Hs[1][: B * 256].isnan().any()


@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("F", (100, 512))
def test_wide_step_rows(F, loss):
    B, N = 129, 3 * 129
    case, y, _ = _case(F, B, loss)
    eng = _engine(F, loss, case.flat)
    other = ex.exact_mlp_case(F, HID, N, F + 7)  # the rest of the table: other lattice rows, exact residuals
    xt = other.x.clone()
    yt = ex.exact_targets(ex.ExactCase(case.lay, case.flat, xt, other.e, case.grad_scale))
    ids = torch.randperm(N, generator=torch.Generator().manual_seed(F))[:B]  # unique: one write per table row
    xt[ids], yt[ids] = case.x, y
    rows = ids.clone()
    rows[5], rows[77], rows[0], rows[1] = ids[4], ids[3], -3, N + 5  # two repeated; two clamped to 0 and N - 1
    got, yg = ex.ExactCase(case.lay, case.flat, xt[rows.clamp(0, N - 1)], None, case.grad_scale), yt[rows.clamp(0, N - 1)]
    assert ex.exactness_violations(got, yg, loss) == []
    ref = ex.mlp_step_fp64(case.flat, got.x, yg, case.grad_scale, loss)
    table = eng.to_input_format(xt.float())
    td = table.to(DEV)
    _check(eng, ref, _step(eng, td, yt, case.grad_scale, rows=rows.to(DEV)), B, f"rows F={F} {loss}")
    assert torch.equal(td.cpu(), table)
    assert torch.equal(eng.X[: B * eng.Fp].view(B, eng.Fp).cpu(), table[rows.clamp(0, N - 1)])


@pytest.mark.parametrize("loss", LOSSES)
def test_wide_step_accumulates(loss):
    case, y, ref = _case(100, 129, loss)
    eng = _engine(100, loss, case.flat)
    x = case.x.float()
    _step(eng, x, y, case.grad_scale)
    _check(eng, ref, _step(eng, x, y, case.grad_scale, zero_grads=False), 129, "accumulated", mult=2.0)
    acc = torch.full((1,), 3.0, device=DEV)
    for k in (1, 2):
        assert _step(eng, x, y, case.grad_scale, loss_into=acc) is acc
        _check(eng, ref, acc, 129, f"loss_into {k}", loss_want=3.0 + k * float(ref["loss_sum"]))


@pytest.mark.parametrize("F", (100, 512))
def test_wide_step_random_against_fp64(F):
    """Same rounding points, another fp32 summation order: at most twice the per-layer route's error."""
    B = 2 * 128 + 37
    g = torch.Generator().manual_seed(F)
    eng = _engine(F, "mse", 0.1 * torch.randn(MlpLayout(F, HID).numel, generator=g))
    x, y = eng.to_input_format(torch.randn(B, F, generator=g)), torch.randn(B, generator=g)
    flat = eng.params.double().cpu()
    for (W, _), (Ws, _) in zip(eng.lay.views(flat)[0], eng.lay.views(eng.shadow.double().cpu())[0]):
        W.copy_(Ws)  # the bf16 shadow weights; fp32 biases and head
    ref = ex.mlp_step_fp64(flat, x[:, :F].double(), y.double(), 1.0 / B)
    err = {}
    for wide in (True, False):
        _step(eng, x, y, 1.0 / B, wide=wide)
        pairs = zip(_blocks(eng.lay, eng.grads.double().cpu()) + [eng.pred[:B].double().cpu()],
                    _blocks(eng.lay, ref["grads"]) + [ref["pred"]])
        err[wide] = [float((a - b).abs().max()) for a, b in pairs]
    print(f"F={F}: max abs error (gW1 gb1 gW2 gb2 ghw ghb pred) wide {err[True]} per-layer {err[False]}")
    assert all(a <= 2 * b for a, b in zip(err[True], err[False])), err


def test_wide_step_refusals():
    case, y, _ = _case(100, 64, "mse")
    eng = _engine(100, "mse", case.flat)
    wl, _, _ = eng.lay.views(eng.shadow)
    pl, hw, hb = eng.lay.views(eng.params)
    x = eng.to_input_format(case.x.float()).to(DEV)
    flat = torch.zeros(64 * 520 + 8, dtype=torch.bfloat16, device=DEV)
    yd, rows = y.float().to(DEV), torch.arange(64, device=DEV)
    for t in (eng.pred, eng.dy, eng.Hs[0]):
        t.fill_(NAN)
    for X, Fp, B, r, why in ((flat, 520, 64, None, "Fp = 520"), (flat, 100, 64, None, "Fp = 100"),
                             (x, eng.Fp, 0, None, "B = 0 rows"), (flat[4:], eng.Fp, 64, None, "16-B aligned"),
                             (x.float(), eng.Fp, 64, None, "contiguous bf16"), (x, eng.Fp, 64, rows, "rows needs Xout")):
        with pytest.raises(RuntimeError, match="mlp2_forward_wide_train: .*" + why):
            eng._C.mlp2_forward_wide_train(X, Fp, wl[0][0], pl[0][1], wl[1][0], pl[1][1], hw, hb, yd, r, None,
                                           eng.Hs[0], eng.M2, eng.pred, eng.dy, eng.grads[:256], eng.grads[256:257],
                                           eng.loss_sum, 1.0, 0.0, B)
        assert eng.pred.isnan().all() and eng.dy.isnan().all() and eng.Hs[0].isnan().all()


def test_mlp_job_on_a_wide_table(tmp_path):
    """The 90-well synthetic table (F = 100) through ``wellflow.submit mlp``: no multi-launch notice."""
    names = "well,field,t,whp,choke,glr,temp,water_cut,dsp,flow"
    types = "string,string,int,float,float,float,float,float,float,float"
    sp = str(tmp_path) + "/"
    r = subprocess.run([sys.executable, "-m", "wellflow.submit", "mlp", names, types, "flow", sp, "--epochs", "2",
                        "--device", "cuda", "--precision", "bf16", "--synth-wells", "90", "--synth-steps", "12"],
                       cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "multi-launch path" not in r.stderr and os.path.exists(sp + "models/mlp.mdl")
    losses = [float(v) for v in re.findall(r"loss[^:\n]*: *([-+.\w]+)", r.stdout)]
    assert losses and bool(torch.tensor(losses).isfinite().all()), r.stdout[-2000:]
