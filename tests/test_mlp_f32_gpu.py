"""The fp32 scoring forward (csrc/mlp_f32.hip) and the precision ``fp32-native`` built on it: float64
bit for bit on two exact lattices, inside the worst-case fp32 bound on random data (where the bf16
route is >= 64 x further off), every refusal, and the predict / response jobs through it."""
import numpy as np
import pytest
import torch

from wellflow.models.mlp import MlpLayout, MLPRegressor, NativeMLP
from wellflow.ops.native import lib

pytestmark = pytest.mark.gpu
DEV, HID, NAN, U = "cuda", (256, 256), float("nan"), 2.0 ** -24
NAMES = "well,field,t,whp,choke,glr,temp,water_cut,dsp,flow"
TYPES = "string,string,int,float,float,float,float,float,float,float"
_ENG = {}


def _engine(F, flat):
    """The engine of width ``F`` (one per width, tile rows x CUs + 1 rows) holding the weights ``flat``."""
    if F not in _ENG:
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        _ENG[F] = NativeMLP(F, HID, lib().MLP_F32_ROWS * cus + 1, device=DEV)
    _ENG[F].params.copy_(flat.float().to(DEV))
    _ENG[F].sync_weights()
    return _ENG[F]


def _fwd64(flat, x, F):
    """float64 forward over MlpLayout weights: (pred, worst-case fp32 error bound of any summation order)."""
    ((W1, b1), (W2, b2)), w3, b3 = MlpLayout(F, HID).views(flat.double())
    x, W1 = x.double(), W1[:, :F]
    h1 = torch.relu(x @ W1.t() + b1)
    e1 = ((F + 7) // 8 * 8 + 1) * U * (x.abs() @ W1.abs().t())  # (Fp + 1) u sum |x w1|, per row and unit
    h2 = torch.relu(h1 @ W2.t() + b2)
    e2 = e1 @ W2.abs().t() + 257 * U * (h1 @ W2.abs().t())
    return h2 @ w3 + b3, e2 @ w3.abs() + 257 * U * (h2 @ w3.abs())


def _run(eng, x, B, ldx):
    """forward_f32 over rows [0, B) of x (cycled), embedded in a NaN buffer of stride ldx, from NaN outputs."""
    buf = torch.full((B + 3, ldx), NAN, device=DEV)
    idx = torch.arange(B) % x.shape[0]
    buf[:B, : x.shape[1]] = x[idx].float().to(DEV)
    before = eng.params.clone()
    eng.pred.fill_(NAN)
    got = eng.forward_f32(buf[:B]).clone()
    assert eng.pred[B:].isnan().all() and torch.equal(eng.params, before)
    return got.cpu(), idx


@pytest.mark.parametrize("F", (5, 8, 33, 64, 65, 100, 264, 509, 512))
def test_coarse_lattice_bit_for_bit(F):
    from wellflow.train import exact as ex

    case = ex.exact_mlp_case(F, HID, 300, 100 * F + 302)
    assert ex.exactness_violations(case, ex.exact_targets(case), "mse") == []
    want = _fwd64(case.flat, case.x, F)[0].float()
    eng = _engine(F, case.flat)
    for B in (1, 63, 64, 65, 129, eng.B):  # eng.B: a workgroup's second tile, a short one
        got, idx = _run(eng, case.x, B, F + 3)
        assert torch.equal(got, want[idx]), f"F={F} B={B}"


@pytest.mark.parametrize("B", (65, 129))
@pytest.mark.parametrize("F", (65, 509))
def test_fine_lattice_bit_for_bit(F, B):
    g = torch.Generator().manual_seed(F + B)
    lay = MlpLayout(F, HID)
    flat = torch.zeros(lay.numel, dtype=torch.float64)
    ((W1, b1), (W2, b2)), w3, b3 = lay.views(flat)
    vals = torch.tensor([-1.0, -0.5, 0.5, 1.0], dtype=torch.float64)
    pick = lambda n: vals[torch.randint(0, 4, (n,), generator=g)]  # noqa: E731
    for W, K in ((W1, F), (W2, 256), (w3.view(1, -1), 256)):
        edges = sorted({0, K - 1} | {k for s in range(32, K, 32) for k in (s - 1, s)})  # every K-slab edge
        for u in range(W.shape[0]):  # <= 4 nonzeros per unit: two slab edges in turn, two anywhere
            pos = [edges[(2 * u) % len(edges)], edges[(2 * u + 1) % len(edges)], *torch.randint(0, K, (2,), generator=g).tolist()]
            W[u, pos] = pick(4)
    for b in (b1, b2, b3):
        b.copy_(0.5 * torch.randint(-1, 2, b.shape, generator=g))
    x = (2 * torch.randint(-2 ** 14, 2 ** 14, (B, F), generator=g) + 1).double() * 2.0 ** -15  # 16 significant bits
    # the premise: every partial sum of every layer, in any order, fits fp32's 24 bits (quantum 2^-16, -17, -18)
    h1 = torch.relu(x @ W1[:, :F].t() + b1)
    h2 = torch.relu(h1 @ W2.t() + b2)
    for terms, b, q in ((x.abs() @ W1[:, :F].abs().t(), b1, -16), (h1 @ W2.abs().t(), b2, -17), (h2 @ w3.abs(), b3, -18)):
        assert float((terms + b.abs()).max()) < 2.0 ** (24 + q)
    want = _fwd64(flat, x, F)[0]
    assert torch.equal(want.float().double(), want)  # fp32-representable
    eng = _engine(F, flat)
    got, _ = _run(eng, x, B, F + 3)
    assert torch.equal(got, want.float())
    bf = eng.forward(eng.to_input_format(x.float()).to(DEV)).cpu()
    assert not torch.equal(bf, want.float())  # a bf16 rounding anywhere shows on this data


@pytest.mark.parametrize("F", (100, 512))
def test_random_data_inside_the_fp32_bound(F):
    g = torch.Generator().manual_seed(F)
    flat = 0.1 * torch.randn(MlpLayout(F, HID).numel, generator=g)
    x = torch.randn(293, F, generator=g)
    eng = _engine(F, flat)
    ref, bound = _fwd64(flat, x, F)
    got, _ = _run(eng, x, 293, F + 3)
    err = (got.double() - ref).abs()
    bf = (eng.forward(eng.to_input_format(x).to(DEV)).cpu().double() - ref).abs().max().item()
    print(f"F={F}: max |pred - fp64| fp32-native {err.max():.3e} (bound {bound.max():.3e}) bf16 {bf:.3e} "
          f"ratio {bf / err.max().item():.0f}")
    assert (err <= bound).all()
    assert bf >= 64 * err.max().item()


def _bad(**kw):
    return kw


@pytest.mark.parametrize("what,change,msg", [
    ("binding", _bad(X=lambda a: a["X"].bfloat16()), "X must be fp32"),
    ("binding", _bad(X=lambda a: a["X"].t()), "X must be contiguous"),
    ("binding", _bad(W2=lambda a: a["W2"].cpu()), "W2 must be a GPU tensor"),
    ("binding", _bad(ldx=lambda a: 99), "ldx = 99"),
    ("binding", _bad(F=lambda a: 0), "F = 0"),
    ("binding", _bad(F=lambda a: 513, ldx=lambda a: 513), "F = 513"),
    ("binding", _bad(B=lambda a: 0), "B = 0"),
    ("binding", _bad(B=lambda a: 65), "X holds"),
    ("binding", _bad(pred=lambda a: a["pred"][:63]), "pred holds 63"),
    ("binding", _bad(W1=lambda a: a["W1"][:255]), "W1 holds"),
    ("binding", _bad(b2=lambda a: a["w3"][:8]), "b2 holds 8"),
    ("engine", lambda e, x: e.forward_f32(x.bfloat16()), "contiguous fp32"),
    ("engine", lambda e, x: e.forward_f32(x.cpu()), "X is on cpu"),
    ("engine", lambda e, x: e.forward_f32(x[:, :99]), "contiguous fp32"),
    ("engine", lambda e, x: e.forward_f32(x[:, :99].contiguous()), "99 values < 100 features"),
    ("engine", lambda e, x: NativeMLP(100, (256, 128), 64, device=DEV).forward_f32(x), r"hidden \(256, 128\)"),
    ("engine", lambda e, x: NativeMLP(513, HID, 64, device=DEV).forward_f32(x), "520 padded input features > 512"),
])
def test_refusals(what, change, msg):
    eng = _engine(100, torch.zeros(MlpLayout(100, HID).numel))
    x = torch.zeros(64, 100, device=DEV)
    eng.pred.fill_(NAN)
    with pytest.raises((RuntimeError, ValueError), match=msg):
        if what == "engine":
            change(eng, x)
        else:
            ((W1, b1), (W2, b2)), w3, b3 = eng.lay.views(eng.params)
            a = dict(X=x, ldx=100, F=100, W1=W1, b1=b1, W2=W2, b2=b2, w3=w3, b3=b3, pred=eng.pred, B=64)
            a.update({k: f(a) for k, f in change.items()})
            eng._C.mlp2_forward_f32(*a.values())
    torch.cuda.synchronize()
    assert eng.pred.isnan().all()


def _saved(tmp_path, wells, name="mlp"):
    from wellflow.data.features import FeaturePipeline
    from wellflow.data.io import load_table
    from wellflow.data.schema import parse_schema
    from wellflow.models import registry
    from wellflow.utils.checkpoint import save_mdl

    schema = parse_schema(NAMES, TYPES)
    table = load_table("synth", schema, synth_wells=wells, synth_steps=12, seed=3)
    pipe = FeaturePipeline(schema, "flow", standardize_target=True).fit(table)
    torch.manual_seed(0)
    ref = MLPRegressor(pipe.n_features, HID)
    p = str(tmp_path / "models" / f"{name}.mdl")
    save_mdl(p, name, registry.keras_layers("mlp", ref), {"features": pipe.state()})
    return schema, table, pipe, ref, p


def test_precision_refusals(tmp_path):
    from wellflow.predict import Predictor
    from wellflow.train.job import run_job

    for name, device, why in (("lstm", "cuda", "not lstm"), ("cnn", "cuda", "not cnn"), ("mlp", "cpu", "GPU only")):
        schema, *_, p = _saved(tmp_path, 4, name)
        with pytest.raises(ValueError, match=f"fp32-native: .*{why}.*--precision fp32 "):
            Predictor.load(p, schema, device=device, precision="fp32-native")
    with pytest.raises(ValueError, match="fp32-native is for scoring only"):
        run_job("mlp", [NAMES, TYPES, "flow", str(tmp_path) + "/", "--precision", "fp32-native", "--synth-wells", "4",
                        "--synth-steps", "50", "--verbose", "0"], log=lambda *a, **k: None)


@pytest.mark.parametrize("wells", (90, 8))  # a categorical column past 64 features; a narrow table
def test_predict_and_response_in_fp32_native(tmp_path, wells):
    from wellflow.data.io import load_table, write_csv
    from wellflow.predict import Predictor, run_predict
    from wellflow.response import ResponseCurves
    from wellflow.scoring import MlpPass, constant

    schema, table, pipe, ref, p = _saved(tmp_path, wells)
    path = str(tmp_path / "data.csv")
    write_csv(table, path, columns=NAMES.split(","))
    table = load_table(path, schema)  # what the job reads
    n, F = len(table["well"]), pipe.n_features
    res = run_predict("mlp", [NAMES, TYPES, "flow", str(tmp_path) + "/", path, "--precision", "fp32-native",
                              "--batch-size", "512"], log=lambda *a, **k: None)
    pred = Predictor.load(p, schema, device="cuda", precision="fp32-native", batch=512)
    ps = MlpPass(pred, table)
    assert res["native"] and pred.native and pred.f32 and ps.on_device and (F > 64) == (wells == 90)
    assert ps.X.dtype == torch.float32 and ps.X.shape == (n, F)
    got = ps.score().cpu()
    assert np.array_equal(res["predictions"], np.asarray(pipe.inverse_target(got.numpy()), np.float32))
    want, bound = _fwd64(ref.to_flat(), torch.from_numpy(pipe.features(table)), F)
    assert ((got.double() - want).abs() <= bound).all()

    out = ResponseCurves(pred).run(table, ["choke"], grids={"choke": [0.2, 0.8]}, by="well")
    assert out["native"] and out["scored"] == n and out["sums"].shape == (3, wells, 3)
    ids = np.unique(np.asarray(table["well"]).astype(str), return_inverse=True)[1]
    for s, tab in enumerate([table] + [constant(table, "choke", np.float32(v)) for v in (0.2, 0.8)]):
        X = torch.from_numpy(pipe.features(tab)).to(DEV)
        own = torch.cat([pred.eng.forward_f32(X[a : a + 512]).clone() for a in range(0, n, 512)]).cpu().numpy()
        v = own.astype(np.float64) * pipe.y_std + pipe.y_mean
        cnt = np.bincount(ids, minlength=wells)
        assert np.array_equal(out["sums"][s, :, 0], cnt)
        for j, w in ((1, v), (2, v * v)):  # two fp64 summations in different orders: n 2^-52 sum |terms|
            err = np.abs(out["sums"][s, :, j] - np.bincount(ids, weights=w, minlength=wells))
            assert (err <= cnt * 2.0 ** -52 * np.bincount(ids, weights=np.abs(w), minlength=wells)).all()
