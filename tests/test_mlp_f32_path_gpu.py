"""The fp32 path-gradient kernel (csrc/mlp_f32_path.hip), path_attr (csrc/score.hip) and the integrated-
gradients job built on them: float64 bit for bit on the exact lattice, inside the worst-case fp32 bound
on random data, every refusal, path_attr against its numpy rule, and the job through the kernel."""
import csv

import numpy as np
import pytest
import torch

from wellflow.integrated import IntegratedGradients, path_alphas, path_attr_host
from wellflow.models.mlp import MlpLayout, MLPRegressor, NativeMLP
from wellflow.ops.native import lib
from wellflow.train import exact as ex

pytestmark = pytest.mark.gpu
DEV, HID, NAN, U = "cuda", (256, 256), float("nan"), 2.0 ** -24
NAMES = "well,field,t,whp,choke,glr,temp,water_cut,dsp,flow"
TYPES = "string,string,int,float,float,float,float,float,float,float"
_ENG = {}


def _engine(F, flat):
    if F not in _ENG:
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        _ENG[F] = NativeMLP(F, HID, lib().MLP_F32_ROWS * cus + 1, device=DEV)
    _ENG[F].params.copy_(flat.float().to(DEV))
    _ENG[F].sync_weights()
    return _ENG[F]


def _path64(flat, x, xb, F, m):
    """float64 (avg, per-step [(alpha, z1, z2, g2, g1)], W1, b1, W2, b2) by the kernel's rule: alpha is the
    fp32 midpoint widened, z1 = (W1 x' + b1) + alpha W1 (x - x'), the masks are z > 0, the mean is over steps."""
    ((W1, b1), (W2, b2)), w3, _ = MlpLayout(F, HID).views(flat.double())
    x, xb, W1 = x.double(), xb.double(), W1[:, :F]
    zb, D = xb @ W1.t() + b1, (x - xb) @ W1.t()
    steps, S = [], torch.zeros_like(D)
    for al in path_alphas(m):
        z1 = zb + float(al) * D
        z2 = torch.relu(z1) @ W2.t() + b2
        g2 = (z2 > 0) * w3
        g1 = (z1 > 0) * (g2 @ W2)
        S = S + g1
        steps.append((float(al), z1, z2, g2, g1))
    return (S @ W1) / m, steps, W1, b1, W2, b2


def _run(eng, x, xb, m, B):
    """path_gradients_f32 over rows [0, B) of x (cycled): X in a NaN buffer of stride F + 3, out (ldg = F + 1)
    and pred from NaN; checks what must stay untouched."""
    F = x.shape[1]
    buf = torch.full((B + 3, F + 3), NAN, device=DEV)
    idx = torch.arange(B) % x.shape[0]
    buf[:B, :F] = x[idx].float().to(DEV)
    out = torch.full((B + 2, F + 1), NAN, device=DEV)
    before = eng.params.clone()
    eng.pred.fill_(NAN)
    avg = eng.path_gradients_f32(buf[:B], xb.float().to(DEV), m, out)
    assert avg.data_ptr() == out.data_ptr() and avg.shape == (B, F + 1)
    assert out[:B, F].isnan().all() and out[B:].isnan().all() and eng.pred.isnan().all()
    assert torch.equal(eng.params, before)
    return out[:B, :F].cpu(), idx


@pytest.mark.parametrize("row0", (False, True))
@pytest.mark.parametrize("m", (1, 4))
@pytest.mark.parametrize("F", (5, 33, 65, 264, 512))
def test_lattice_bit_for_bit(F, m, row0):
    case = ex.exact_mlp_case(F, HID, 300, 100 * F + 302)
    xb = case.x[0] if row0 else torch.zeros(F)
    want = _path64(case.flat, case.x, xb, F, m)[0]
    assert torch.equal(want.float().double(), want)  # fp32-representable
    eng = _engine(F, case.flat)
    for B in (1, 63, 64, 65, 129, eng.B):  # eng.B: a workgroup's second tile, a one-row tile
        got, idx = _run(eng, case.x, xb, m, B)
        assert torch.equal(got, want.float()[idx]), f"F={F} m={m} B={B}"


@pytest.mark.parametrize("F,m", ((13, 3), (40, 2)))
def test_random_data_inside_the_fp32_bound(F, m):
    """The bound, from the kernel's operation order (U = 2^-24, Fp = F padded to 8). d = fl(x - x') carries
    U |x - x'|; D = W1 d is an Fp-term fp32 sum, so |D - D*| <= (Fp + 1) U |x - x'| @ |W1|^T; zb is an
    Fp-term fmaf chain plus the add of b1: (Fp + 1) U (|x'| @ |W1|^T + |b1|); z1_j = fmaf(alpha_j, D, zb)
    rounds once more (alpha_j is the reference's own fp32 value). Together, to first order,
    e1_j = (Fp + 3) U (|x'| @ |W1|^T + |b1| + alpha_j |x - x'| @ |W1|^T). Layer 2 is a 256-term sum plus b2:
    e2_j = e1_j @ |W2|^T + 257 U (h1_j @ |W2|^T + |b2|). A row is kept when no mask can flip at any step
    (|z| > e everywhere). For a kept row the masks are the reference's, G2 is exact, G1_j is a 256-term
    sum (257 U |g2_j| @ |W2| under the mask), S adds m values in order and is scaled once ((m + 1) U
    mean_j |g1_j|), and the last product is a 256-term sum of S: per step the gradient test's bound,
    averaged, plus (m + 1) U (mean_j |g1_j|) @ |W1|."""
    g = torch.Generator().manual_seed(F)
    flat = 0.1 * torch.randn(MlpLayout(F, HID).numel, generator=g)
    x = torch.randn(293, F, generator=g)
    xb = x.mean(0)
    ref, steps, W1, b1, W2, b2 = _path64(flat, x, xb, F, m)
    Fp, xa, da = (F + 7) // 8 * 8, xb.double().abs(), (x.double() - xb.double()).abs()
    keep, bound, g1m = torch.ones(293, dtype=torch.bool), 0.0, 0.0
    for al, z1, z2, g2, g1 in steps:
        e1 = (Fp + 3) * U * (xa @ W1.abs().t() + b1.abs() + al * (da @ W1.abs().t()))
        e2 = e1 @ W2.abs().t() + 257 * U * (torch.relu(z1) @ W2.abs().t() + b2.abs())
        keep &= (z1.abs() > e1).all(1) & (z2.abs() > e2).all(1)
        eg1 = 257 * U * (g2.abs() @ W2.abs()) * (z1 > 0)
        bound = bound + (eg1 @ W1.abs() + 257 * U * (g1.abs() @ W1.abs())) / m
        g1m = g1m + g1.abs() / m
    bound = bound + (m + 1) * U * (g1m @ W1.abs())
    assert (~keep).float().mean() <= 0.20
    got, _ = _run(_engine(F, flat), x, xb, m, 293)
    err = (got.double() - ref).abs()[keep]
    print(f"F={F} m={m}: {int((~keep).sum())} of 293 rows excluded, worst error/bound "
          f"{(err / bound[keep]).max():.3f}, bound max {bound.max():.2e}, median |avg| {ref.abs().median():.3f}")
    assert (err <= bound[keep]).all()


@pytest.mark.parametrize("call,msg", [
    (lambda e, x, b, o: NativeMLP(100, (256, 128), 64, device=DEV).path_gradients_f32(x, b, 4, o), r"hidden \(256, 128\)"),
    (lambda e, x, b, o: NativeMLP(513, HID, 64, device=DEV).path_gradients_f32(x, b, 4, o), "520 padded input features > 512"),
    (lambda e, x, b, o: e.path_gradients_f32(x.bfloat16(), b, 4, o), "contiguous fp32"),
    (lambda e, x, b, o: e.path_gradients_f32(x[:, :101], b, 4, o), "contiguous fp32"),
    (lambda e, x, b, o: e.path_gradients_f32(x, b, 4, o[:, :99].contiguous()), "needs >= 64 rows of >= 100 values"),
    (lambda e, x, b, o: e.path_gradients_f32(torch.zeros(e.B + 1, 100, device=DEV), b, 4), "rows \\(the engine's batch"),
    (lambda e, x, b, o: e.path_gradients_f32(x, b, 4, o.cpu()), "out is on cpu"),
    (lambda e, x, b, o: e.path_gradients_f32(x, b.cpu(), 4, o), "baseline is on cpu"),
    (lambda e, x, b, o: e.path_gradients_f32(x, b[:99], 4, o), "baseline holds 99 values"),
    (lambda e, x, b, o: e.path_gradients_f32(x, b.double(), 4, o), "baseline must be a contiguous fp32"),
    (lambda e, x, b, o: e.path_gradients_f32(x, b, 0, o), "steps = 0"),
    (lambda e, x, b, o: e.path_gradients_f32(x, b, 1025, o), "steps = 1025"),
    (lambda e, x, b, o: e._C.mlp2_path_grad_f32(x, 102, 100, b, *e._views(), 1025, o, 100, 64), "steps = 1025"),
    (lambda e, x, b, o: e._C.mlp2_path_grad_f32(x, 102, 100, b, *e._views(), 4, o, 99, 64), "ldg = 99"),
])
def test_refusals(call, msg):
    eng = _engine(100, torch.zeros(MlpLayout(100, HID).numel))
    ((W1, b1), (W2, b2)), w3, _ = eng.lay.views(eng.params)
    eng._views = lambda: (W1, b1, W2, b2, w3)
    x, out = torch.zeros(64, 102, device=DEV), torch.full((64, 100), NAN, device=DEV)
    eng.pred.fill_(NAN)
    with pytest.raises((RuntimeError, ValueError), match=msg):
        call(eng, x, torch.zeros(100, device=DEV), out)
    torch.cuda.synchronize()
    assert eng.pred.isnan().all() and out.isnan().all()


def test_path_attr_bit_for_bit():
    g = torch.Generator().manual_seed(7)
    F, n, cut = 70, 203, 129
    X, avg, xb = torch.randn(n, F + 2, generator=g), torch.randn(n, F, generator=g), torch.randn(F, generator=g)
    avg[5, 40] = NAN
    off, size = np.asarray([0, 3, 3, 20, 69, 12], np.int32), np.asarray([3, 0, 17, 49, 1, 58], np.int32)  # 0-size; across 32 and 64
    want = path_attr_host(X[:, :F].numpy(), avg.numpy(), xb.numpy(), off, size)
    phi = torch.full((len(off), n), NAN, dtype=torch.float64, device=DEV)
    o, s = torch.from_numpy(off).to(DEV), torch.from_numpy(size).to(DEV)
    for a, b in ((0, cut), (cut, n)):  # two pieces fill one table
        lib().path_attr(X[a:b].contiguous().to(DEV), avg[a:b].contiguous().to(DEV), xb.to(DEV), F, o, s, phi, a)
    assert np.array_equal(phi.cpu().numpy(), want, equal_nan=True) and (want[1] == 0.0).all()
    assert np.isnan(want[3, 5]) and np.isnan(want[5, 5]) and np.isfinite(want[:3]).all()
    with pytest.raises(RuntimeError, match="span 0"):
        lib().path_attr(X.to(DEV), avg.to(DEV), xb.to(DEV), F, o, torch.full_like(s, F + 1), phi, 0)


def test_ig_job_on_the_device(tmp_path):
    from wellflow.data.features import FeaturePipeline
    from wellflow.data.io import load_table, write_csv
    from wellflow.data.schema import parse_schema
    from wellflow.explain import run_explain
    from wellflow.models import registry
    from wellflow.predict import Predictor
    from wellflow.utils.checkpoint import save_mdl

    schema = parse_schema(NAMES, TYPES)
    table = load_table("synth", schema, synth_wells=8, synth_steps=100, seed=3)
    pipe = FeaturePipeline(schema, "flow", standardize_target=True).fit(table)
    torch.manual_seed(0)
    ref = MLPRegressor(pipe.n_features, HID)
    glr = pipe.n_features - len(pipe.continuous) + list(pipe.continuous).index("glr")
    with torch.no_grad():
        next(ref.parameters())[:, glr] = 0.0  # the model does not read glr
    mdl = str(tmp_path / "models" / "mlp.mdl")
    save_mdl(mdl, "mlp", registry.keras_layers("mlp", ref), {"features": pipe.state()})
    path = str(tmp_path / "data.csv")
    write_csv(table, path, columns=NAMES.split(","))
    table = load_table(path, schema)  # what the job reads
    n = len(table["well"])

    pred = Predictor.load(mdl, schema, device="cuda", precision="fp32-native", batch=256)
    job = IntegratedGradients(pred, steps=8, piece_rows=512)  # two pieces, chunks of 256 rows
    out = job.run(table)
    cols = out["columns"]
    assert out["native"] and n == 800 and out["phi"].shape == (len(cols), n) and "glr" in cols
    # the replay: the kernel over host-assembled rows, then path_attr_host and the float64 formulas
    Xh, xb = pipe.features(table), job.baseline_row(table, n)
    X, xbd = torch.from_numpy(Xh).to(DEV), torch.from_numpy(xb).to(DEV)
    avg = torch.cat([pred.eng.path_gradients_f32(X[a : a + 256], xbd, 8).clone() for a in range(0, n, 256)])
    p = torch.cat([pred.eng.forward_f32(X[a : a + 256]).clone() for a in range(0, n, 256)]).cpu().numpy()
    phi = path_attr_host(Xh, avg.cpu().numpy(), xb, *job.spans()) * pipe.y_std
    v = p.astype(np.float64) * pipe.y_std + pipe.y_mean
    base = float(pred.eng.forward_f32(xbd[None, :]).cpu()[0]) * pipe.y_std + pipe.y_mean
    total = np.zeros(n)
    for k in range(len(phi)):
        total = total + phi[k]
    assert np.array_equal(out["prediction"], v) and np.array_equal(out["phi"], phi) and (out["base"] == base).all()
    assert np.array_equal(out["residual"], v - base - total)
    assert (out["phi"][cols.index("glr")] == 0.0).all() and np.abs(out["phi"][cols.index("whp")]).max() > 0

    res = run_explain("mlp", [NAMES, TYPES, "flow", str(tmp_path) + "/", path, "--method", "ig", "--steps", "8",
                              "--batch-size", "256"], log=lambda *a, **k: None)
    assert res["native"] and res["out"].endswith("explain/mlp.csv")
    with open(res["out"]) as f:
        rows = list(csv.reader(f))
    assert rows[0] == NAMES.split(",") + ["prediction", "base"] + [f"phi_{c}" for c in cols] + ["residual"]
    back = np.asarray([[float(c) for c in r[len(schema.names):]] for r in rows[1:]])
    assert np.array_equal(back[:, 0], out["prediction"]) and np.array_equal(back[:, 1], out["base"])
    assert np.array_equal(back[:, 2:-1].T, out["phi"]) and np.array_equal(back[:, -1], out["residual"])

    # measurements, not conditions: the quadrature error against steps, and the oracle route against the kernel
    r64 = IntegratedGradients(pred, steps=64).run(table)
    ora = IntegratedGradients(Predictor.load(mdl, schema, device="cuda", precision="fp32"), steps=8,
                              note=lambda s: None).run(table)
    assert not ora["native"]
    rel = np.abs(ora["phi"] - out["phi"]) / np.maximum(np.abs(out["phi"]), 1e-300)
    rel = rel[np.abs(out["phi"]) > 0]
    print(f"max |residual| at 8 steps {np.abs(out['residual']).max():.3e}, at 64 steps {np.abs(r64['residual']).max():.3e}; "
          f"oracle route vs kernel, relative phi difference: median {np.median(rel):.3e}, max {rel.max():.3e}")
