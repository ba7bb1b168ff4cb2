"""The fp32 input-gradient kernel (csrc/mlp_f32_grad.hip) and the sensitivity job built on it: float64
bit for bit on the exact lattice, inside the worst-case fp32 bound on random data, the gradient
follows the weights, every refusal, and the job through the kernel."""
import csv

import numpy as np
import pytest
import torch

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


def _grad64(flat, x, F):
    """float64 (dx, z1, z2, |g2|, |g1|, W1, W2) of the float64 reference; the ReLU masks are z > 0."""
    ((W1, b1), (W2, b2)), w3, _ = MlpLayout(F, HID).views(flat.double())
    x, W1 = x.double(), W1[:, :F]
    z1 = x @ W1.t() + b1
    z2 = torch.relu(z1) @ W2.t() + b2
    g2 = (z2 > 0) * w3
    g1 = (z1 > 0) * (g2 @ W2)
    return g1 @ W1, z1, z2, g2, g1, W1, W2


def _run(eng, x, B):
    """input_gradients_f32 over rows [0, B) of x (cycled): X in a NaN buffer of stride F + 3, dX (ldg = F + 1)
    and pred from NaN; checks what must stay untouched and that pred has forward_f32's bits."""
    F = x.shape[1]
    buf = torch.full((B + 3, F + 3), NAN, device=DEV)
    idx = torch.arange(B) % x.shape[0]
    buf[:B, :F] = x[idx].float().to(DEV)
    out = torch.full((B + 2, F + 1), NAN, device=DEV)
    before = eng.params.clone()
    eng.pred.fill_(NAN)
    p, dx = eng.input_gradients_f32(buf[:B], out)
    p = p.clone()
    assert dx.data_ptr() == out.data_ptr() and dx.shape == (B, F + 1)
    assert out[:B, F].isnan().all() and out[B:].isnan().all() and eng.pred[B:].isnan().all()
    assert torch.equal(eng.params, before)
    assert torch.equal(p, eng.forward_f32(buf[:B])), f"pred differs from forward_f32 at B={B}"
    return out[:B, :F].cpu(), idx


@pytest.mark.parametrize("F", (5, 8, 33, 64, 65, 100, 264, 509, 512))
def test_lattice_bit_for_bit(F):
    case = ex.exact_mlp_case(F, HID, 300, 100 * F + 302)
    want = _grad64(case.flat, case.x, F)[0]
    assert torch.equal(want.float().double(), want)  # fp32-representable
    eng = _engine(F, case.flat)
    for B in (1, 63, 64, 65, 129, eng.B):  # eng.B: a workgroup's second tile, a one-row tile
        got, idx = _run(eng, case.x, B)
        assert torch.equal(got, want.float()[idx]), f"F={F} B={B}"


@pytest.mark.parametrize("F", (13, 72))
def test_random_data_inside_the_fp32_bound(F):
    g = torch.Generator().manual_seed(F)
    flat = 0.1 * torch.randn(MlpLayout(F, HID).numel, generator=g)
    x = torch.randn(293, F, generator=g)
    ref, z1, z2, g2, g1, W1, W2 = _grad64(flat, x, F)
    xa, h1 = x.double().abs(), torch.relu(z1)
    e1 = ((F + 7) // 8 * 8 + 1) * U * (xa @ W1.abs().t())  # as _fwd64 of tests/test_mlp_f32_gpu.py
    e2 = e1 @ W2.abs().t() + 257 * U * (h1 @ W2.abs().t())
    keep = (z1.abs() > e1).all(1) & (z2.abs() > e2).all(1)  # no mask of the row may legitimately flip
    assert (~keep).float().mean() <= 0.15
    eg1 = 257 * U * (g2.abs() @ W2.abs()) * (z1 > 0)
    bound = eg1 @ W1.abs() + 257 * U * (g1.abs() @ W1.abs())
    got, _ = _run(_engine(F, flat), x, 293)
    err = (got.double() - ref).abs()[keep]
    print(f"F={F}: {int((~keep).sum())} of 293 rows excluded, worst error/bound "
          f"{(err / bound[keep]).max():.3f}, bound max {bound.max():.2e}, median |grad| {ref.abs().median():.3f}")
    assert (err <= bound[keep]).all()


def test_gradient_follows_the_weights():
    F = 65
    a, b = (ex.exact_mlp_case(F, HID, 300, s) for s in (100 * F + 302, 100 * F + 303))
    assert not torch.equal(a.flat, b.flat)
    for case in (a, b):  # the second call must not see anything kept from the first
        got, idx = _run(_engine(F, case.flat), case.x, 129)
        assert torch.equal(got, _grad64(case.flat, case.x, F)[0].float()[idx])


@pytest.mark.parametrize("call,msg", [
    (lambda e, x, o: NativeMLP(100, (256, 128), 64, device=DEV).input_gradients_f32(x, o), r"hidden \(256, 128\)"),
    (lambda e, x, o: NativeMLP(513, HID, 64, device=DEV).input_gradients_f32(x, o), "520 padded input features > 512"),
    (lambda e, x, o: e.input_gradients_f32(x.bfloat16(), o), "contiguous fp32"),
    (lambda e, x, o: e.input_gradients_f32(x[:, :101], o), "contiguous fp32"),
    (lambda e, x, o: e.input_gradients_f32(x, o[:, :99].contiguous()), "needs >= 64 rows of >= 100 values"),
    (lambda e, x, o: e.input_gradients_f32(torch.zeros(e.B + 1, 100, device=DEV)), "rows \\(the engine's batch"),
    (lambda e, x, o: e.input_gradients_f32(x, o.cpu()), "out is on cpu"),
    (lambda e, x, o: e._C.mlp2_forward_grad_f32(x, 102, 100, *e._views(), e.pred, o, 99, 64), "ldg = 99"),
    (lambda e, x, o: e._C.mlp2_forward_grad_f32(x, 102, 100, *e._views(), e.pred, o[:63], 100, 64), "dX holds"),
])
def test_refusals(call, msg):
    eng = _engine(100, torch.zeros(MlpLayout(100, HID).numel))
    ((W1, b1), (W2, b2)), w3, b3 = eng.lay.views(eng.params)
    eng._views = lambda: (W1, b1, W2, b2, w3, b3)
    x, out = torch.zeros(64, 102, device=DEV), torch.full((64, 100), NAN, device=DEV)
    eng.pred.fill_(NAN)
    with pytest.raises((RuntimeError, ValueError), match=msg):
        call(eng, x, out)
    torch.cuda.synchronize()
    assert eng.pred.isnan().all() and out.isnan().all()


def test_sensitivity_job_on_the_device(tmp_path):
    from wellflow.data.features import FeaturePipeline
    from wellflow.data.io import load_table, write_csv
    from wellflow.data.schema import parse_schema
    from wellflow.models import registry
    from wellflow.predict import Predictor
    from wellflow.sensitivity import Sensitivity, run_sensitivity
    from wellflow.utils.checkpoint import save_mdl

    schema = parse_schema(NAMES, TYPES)
    table = load_table("synth", schema, synth_wells=8, synth_steps=100, seed=3)
    pipe = FeaturePipeline(schema, "flow", standardize_target=True).fit(table)
    torch.manual_seed(0)
    ref = MLPRegressor(pipe.n_features, HID)
    save_mdl(str(tmp_path / "models" / "mlp.mdl"), "mlp", registry.keras_layers("mlp", ref), {"features": pipe.state()})
    path = str(tmp_path / "data.csv")
    write_csv(table, path, columns=NAMES.split(","))
    table = load_table(path, schema)  # what the job reads
    n, cols = len(table["well"]), ["whp", "choke", "glr"]

    pred = Predictor.load(str(tmp_path / "models" / "mlp.mdl"), schema, device="cuda", precision="fp32-native", batch=256)
    out = Sensitivity(pred, piece_rows=512).run(table, cols)  # two pieces, chunks of 256 rows
    assert out["native"] and out["columns"] == cols and out["grad"].shape == (3, n) and n == 800
    # the replay: the kernel over host-assembled rows, then the job's float64 formulas in numpy
    X = torch.from_numpy(pipe.features(table)).to(DEV)
    p, g = (torch.cat(v).cpu().numpy().astype(np.float64) for v in zip(*(
        [t.clone() for t in pred.eng.input_gradients_f32(X[a : a + 256])] for a in range(0, n, 256))))
    v = p * pipe.y_std + pipe.y_mean
    fcol = [pipe.n_features - len(pipe.continuous) + list(pipe.continuous).index(c) for c in cols]
    std = pipe.scale()[1].astype(np.float64)
    assert np.array_equal(out["prediction"], v)
    for k, c in enumerate(cols):
        grad = g[:, fcol[k]] * pipe.y_std / std[list(pipe.continuous).index(c)]
        assert np.array_equal(out["grad"][k], grad)
        with np.errstate(all="ignore"):
            assert np.array_equal(out["elast"][k], grad * np.asarray(table[c], np.float32).astype(np.float64) / v, equal_nan=True)

    res = run_sensitivity("mlp", [NAMES, TYPES, "flow", str(tmp_path) + "/", path, "--columns", ",".join(cols),
                                  "--batch-size", "256"], log=lambda *a, **k: None)
    assert res["native"] and res["out"].endswith("sensitivity/mlp.csv")
    with open(res["out"]) as f:
        rows = list(csv.reader(f))
    assert rows[0] == NAMES.split(",") + ["prediction"] + [f"{s}_{c}" for c in cols for s in ("grad", "elast")]
    back = np.asarray([[float(c) for c in r[len(schema.names):]] for r in rows[1:]])
    assert np.array_equal(back[:, 0], out["prediction"])
    assert np.array_equal(back[:, 1::2].T, out["grad"]) and np.array_equal(back[:, 2::2].T, out["elast"], equal_nan=True)

    # a measurement, not a condition: the fp32 oracle route (torch.autograd) against the kernel
    ora = Sensitivity(Predictor.load(str(tmp_path / "models" / "mlp.mdl"), schema, device="cuda", precision="fp32"),
                      note=lambda s: None).run(table, cols)
    assert not ora["native"]
    rel = np.abs(ora["grad"] - out["grad"]) / np.maximum(np.abs(out["grad"]), 1e-300)
    print(f"oracle route vs kernel: median relative grad difference {np.median(rel):.3e}, max {rel.max():.3e}, "
          f"rows with a relative difference > 1e-3: {(rel.max(0) > 1e-3).mean():.4f}")
