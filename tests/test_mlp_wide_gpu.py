"""The fused scoring forward for 65-512 features (csrc/mlp_wide.hip): float64 bit for bit on exact
data (wellflow/train/exact.py), row-independent and no noisier than the per-layer route on random data."""
import numpy as np
import pytest
import torch

from wellflow.ops.native import lib  # lib().MLP_WIDE_ROWS: the kernel's row tile R

pytestmark = pytest.mark.gpu
DEV = "cuda"
HID = (256, 256)
NAN = float("nan")
F_EXACT = (65, 72, 96, 100, 128, 136, 264, 509, 512)
_ENG = {}


def _engine(F, flat):
    """The engine of width ``F`` (one per width, R * CUs + 1 rows) with the weights ``flat`` (MlpLayout order)."""
    from wellflow.models.mlp import NativeMLP

    if F not in _ENG:
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        _ENG[F] = NativeMLP(F, HID, lib().MLP_WIDE_ROWS * cus + 1, device=DEV)
    _ENG[F].params.copy_(flat.float().to(DEV))
    _ENG[F].sync_weights()
    return _ENG[F]


def _random(F, rows):  # (engine with seeded normal weights, seeded normal rows in the bf16 input format)
    from wellflow.models.mlp import MlpLayout

    g = torch.Generator().manual_seed(F)
    eng = _engine(F, 0.1 * torch.randn(MlpLayout(F, HID).numel, generator=g))
    return eng, eng.to_input_format(torch.randn(rows, F, generator=g)).to(DEV)


def _args(eng):
    wl, _, _ = eng.lay.views(eng.shadow)
    pl, hw, hb = eng.lay.views(eng.params)
    return wl[0][0], pl[0][1], wl[1][0], pl[1][1], hw, hb


def _route(eng, x, wide):
    """forward() on one route from NaN-filled outputs: (pred copy, were H1 / H2 left untouched)."""
    for t in (eng.pred, *eng.Hs):
        t.fill_(NAN)
    eng.wide_fwd = wide
    got = eng.forward(x).clone()
    eng.wide_fwd = True
    assert eng.pred[x.shape[0]:].isnan().all()
    return got, all(bool(h.isnan().all()) for h in eng.Hs)


def _exact(F, B):
    from wellflow.train import exact as ex

    case = ex.exact_mlp_case(F, HID, B, 100 * F + B + 2)
    y = ex.exact_targets(case)
    assert ex.exactness_violations(case, y, "mse") == []
    return case, ex.mlp_step_fp64(case.flat, case.x, y, case.grad_scale)["pred"].float()


@pytest.mark.parametrize("F", F_EXACT)
def test_wide_forward_exact(F):
    case, want = _exact(F, 300)
    eng = _engine(F, case.flat)
    R = lib().MLP_WIDE_ROWS
    big = (eng.B,) if F in (72, 512) else ()  # R * CUs + 1: a workgroup's second tile, a short one
    for B in (1, 63, 64, 65, R - 1, R, R + 1, 300) + big:
        idx = torch.arange(B) % 300  # rows are independent: the 300 exact rows, repeated
        table = torch.full((B + 16, eng.Fp), NAN, dtype=torch.bfloat16, device=DEV)
        table[8 : 8 + B] = eng.to_input_format(case.x[idx].float()).to(DEV)  # zero-padded to Fp
        for wide in (True, False):
            got, untouched = _route(eng, table[8 : 8 + B], wide)
            assert torch.equal(got.cpu(), want[idx]), f"F={F} B={B} wide={wide}"
            assert untouched == wide, f"F={F} B={B} wide={wide}: H1 / H2 in HBM"
            assert wide or not any(bool(h[: B * 256].isnan().any()) for h in eng.Hs)


@pytest.mark.parametrize("F", (5, 32, 40, 64))
def test_wide_forward_binding_below_65(F):
    case, want = _exact(F, 65)
    eng = _engine(F, case.flat)
    pred = torch.full((65 + 8,), NAN, device=DEV)
    eng._C.mlp2_forward_wide(eng.to_input_format(case.x.float()).to(DEV), eng.Fp, *_args(eng), pred, 65)
    assert torch.equal(pred[:65].cpu(), want) and pred[65:].isnan().all()


@pytest.mark.parametrize("F", (100, 512))
def test_wide_forward_rows_are_independent(F):
    eng, x = _random(F, 2 * lib().MLP_WIDE_ROWS + 37)
    R, B = lib().MLP_WIDE_ROWS, x.shape[0]
    whole, untouched = _route(eng, x, True)
    assert untouched and whole.isfinite().all()
    for r in (0, R - 1, R, 2 * R, B - 1):
        assert torch.equal(eng.forward(x[r : r + 1]), whole[r : r + 1]), r
    for a, b in ((R - 1, B), (0, B // 2), (B // 2, B)):
        assert torch.equal(eng.forward(x[a:b]), whole[a:b])


@pytest.mark.parametrize("F", (100, 512))
def test_wide_forward_random_against_fp64(F):
    """Same rounding points, another fp32 summation order: at most twice the per-layer route's error."""
    eng, x = _random(F, 2 * lib().MLP_WIDE_ROWS + 37)
    W1, b1, W2, b2, hw, hb = (t.double() for t in _args(eng))  # the bf16 shadow weights, fp32 biases and head
    h = torch.relu(x.double() @ W1.t() + b1).bfloat16().double()
    ref = torch.relu(h @ W2.t() + b2).bfloat16().double() @ hw + hb
    err = {wide: (_route(eng, x, wide)[0].double() - ref).abs().max().item() for wide in (True, False)}
    print(f"F={F}: max |pred - fp64| wide {err[True]:.3e} per-layer {err[False]:.3e}")
    assert err[True] <= 2 * err[False], err


def test_wide_forward_refusals():
    eng, x = _random(100, 64)
    pred = torch.full((64,), NAN, device=DEV)
    flat = torch.zeros(64 * 520 + 8, dtype=torch.bfloat16, device=DEV)
    for X, Fp, B in ((flat, 520, 64), (flat, 100, 64), (x, eng.Fp, 0), (flat[4:], eng.Fp, 64), (x.float(), eng.Fp, 64)):
        with pytest.raises(RuntimeError, match="mlp2_forward_wide"):
            eng._C.mlp2_forward_wide(X, Fp, *_args(eng), pred, B)
        assert pred.isnan().all()


def test_predict_job_on_a_wide_table(tmp_path):
    from wellflow.data.features import FeaturePipeline
    from wellflow.data.io import load_table
    from wellflow.data.schema import parse_schema
    from wellflow.models import registry
    from wellflow.models.mlp import MLPRegressor
    from wellflow.predict import Predictor
    from wellflow.utils.checkpoint import save_mdl

    schema = parse_schema("well,field,t,whp,choke,glr,temp,water_cut,dsp,flow",
                          "string,string,int,float,float,float,float,float,float,float")
    table = load_table("synth", schema, synth_wells=90, synth_steps=12, seed=3)
    pipe = FeaturePipeline(schema, "flow", standardize_target=True).fit(table)
    assert pipe.n_features == 100  # 90 well labels: the job reaches the wide kernel through predict_table
    torch.manual_seed(0)
    p = str(tmp_path / "models" / "mlp.mdl")
    save_mdl(p, "mlp", registry.keras_layers("mlp", MLPRegressor(pipe.n_features, HID)), {"features": pipe.state()})
    pred = Predictor.load(p, schema, device="cuda", precision="bf16", batch=512)
    pred.predict_table(table)  # builds the engine
    eng = pred.eng
    eng.Hs[0].fill_(NAN), eng.Hs[1].fill_(NAN)
    got = pred.predict_table(table)  # 1080 rows: two chunks of 512 and one of 56
    assert pred.native and all(bool(h.isnan().all()) for h in eng.Hs)
    Xh = eng.to_input_format(torch.from_numpy(pipe.transform(table)[0])).to(DEV)
    host = torch.cat([eng.forward(Xh[a : a + 512]).clone() for a in range(0, len(got), 512)]).cpu().numpy()
    assert np.isfinite(got).all() and np.array_equal(got, np.asarray(pipe.inverse_target(host), np.float32))
