"""Integrated gradients on the CPU (wellflow/integrated.py): path_attr_host against a per-element loop, the
oracle route on an affine network, Gilbert's closed form, and the refusals of ``explain --method ig``."""
import numpy as np
import pytest
import torch

from wellflow.data.features import FeaturePipeline
from wellflow.data.io import load_table, write_csv
from wellflow.data.schema import parse_schema
from wellflow.explain import run_explain
from wellflow.integrated import IntegratedGradients, path_attr_host
from wellflow.models import registry
from wellflow.models.mlp import MLPRegressor
from wellflow.predict import Predictor
from wellflow.utils.checkpoint import save_mdl

NAMES = "well,field,t,whp,choke,glr,temp,water_cut,dsp,flow"
TYPES = "string,string,int,float,float,float,float,float,float,float"
U = 2.0 ** -24


def _saved(tmp_path, name="mlp", edit=None):
    schema = parse_schema(NAMES, TYPES)
    table = load_table("synth", schema, synth_wells=3, synth_steps=34, seed=3)
    p = str(tmp_path / "models" / f"{name}.mdl")
    if name == "gilbert":
        save_mdl(p, name, [("Gilbert", [torch.tensor([17.4, 0.5, 2.0])])], {"correlation": "ros", "glr_unit": "scf"})
        return schema, table, None, None, p
    pipe = FeaturePipeline(schema, "flow", standardize_target=True).fit(table)
    torch.manual_seed(0)
    ref = MLPRegressor(pipe.n_features, (256, 256))
    if edit:
        edit(ref)
    save_mdl(p, name, registry.keras_layers(name, ref), {"features": pipe.state()})
    return schema, table, pipe, ref, p


def test_path_attr_host_against_a_loop():
    r = np.random.default_rng(1)
    X, avg, xb = (r.standard_normal(s).astype(np.float32) for s in ((9, 40), (9, 40), (40,)))
    off, size = [0, 2, 2, 30], [2, 0, 35, 10]
    got = path_attr_host(X, avg, xb, off, size)
    for k in range(4):
        for i in range(9):
            s = 0.0
            for f in range(off[k], off[k] + size[k]):
                s = s + (float(X[i, f]) - float(xb[f])) * float(avg[i, f])
            assert got[k, i] == s
    assert (got[1] == 0.0).all()


def test_baseline_rows_against_the_pipeline(tmp_path):
    """``mean`` against the mean of the pipeline's own fp32 feature rows, taken in float64: the two differ by
    the fp32 rounding of each row's standardised value (U relative to |x| per row, so U mean|x|) and of the
    result (U |mean|); one-hot features are exact in both. ``N`` is the pipeline's row N, bit for bit."""
    schema, table, pipe, _, p = _saved(tmp_path)
    table = dict(table)
    table["well"] = np.asarray(table["well"]).copy()
    table["well"][:7] = "never-seen"  # the pipeline's unknown-label rule is on the path
    pred = Predictor.load(p, schema, device="cpu", precision="fp32")
    X = pipe.features(table).astype(np.float64)
    got = IntegratedGradients(pred).baseline_row(table, len(X))
    assert got.dtype == np.float32 and got.shape == (pipe.n_features,)
    assert (np.abs(got - X.mean(0)) <= 2 * U * (np.abs(X).mean(0) + np.abs(X.mean(0)))).all()
    nc = len(pipe.continuous)
    assert (got[:-nc] == X.mean(0)[:-nc].astype(np.float32)).all() and got[:-nc].sum() < 2.0  # 7 unknown rows: no 1 anywhere
    for i in (0, 57, len(X) - 1):
        assert np.array_equal(IntegratedGradients(pred, baseline=i).baseline_row(table, len(X)), pipe.features(table)[i])


@pytest.mark.parametrize("steps", (1, 5))
def test_oracle_route_on_an_affine_network(tmp_path, steps):
    """Biases of 1 against weights scaled by 0.01 keep every unit active on every path (|W1 x| and |W2 h1|
    stay far below 1 on standardised rows, asserted), so the network is affine there: the gradient is
    w_eff = W1^T W2^T w3 everywhere, phi_f = (x_f - x'_f) w_eff_f and the residual is rounding only, at any
    steps. Its bound: the fp32 forward of a row is three sums of F, 256 and 256 terms plus three bias adds,
    to first order (F + 515) U A(x) with A(x) = |w3| . (|W2| (|W1| |x| + |b1|) + |b2|) + |b3|; the fp32
    gradient is two 256-term products, 514 U |W1|^T |W2|^T |w3|, times |x - x'|. The float64 steps add a few
    2^-53 of the terms' magnitudes."""
    def affine(ref):
        with torch.no_grad():
            for lin in ref.linears():
                lin.weight.mul_(0.01)
                lin.bias.fill_(1.0)

    schema, table, pipe, ref, p = _saved(tmp_path, edit=affine)
    notes = []
    out = IntegratedGradients(Predictor.load(p, schema, device="cpu", precision="fp32"), steps=steps,
                              note=notes.append).run(table)
    assert not out["native"] and len(notes) == 1 and "oracle" in notes[0]
    (W1, b1, W2, b2, w3, b3) = (t.detach().double().numpy() for t in ref.parameters())
    job = IntegratedGradients(Predictor.load(p, schema, device="cpu", precision="fp32"), steps=steps)
    X, xb = pipe.features(table).astype(np.float64), job.baseline_row(table, len(table["well"])).astype(np.float64)
    assert (np.abs(X) @ np.abs(W1).T).max() < 0.9 and 2 * np.abs(W2).sum(1).max() < 0.9
    A = lambda x: (np.abs(x) @ np.abs(W1).T + np.abs(b1)) @ np.abs(W2).T @ np.abs(w3[0]) + np.abs(b2) @ np.abs(w3[0]) + abs(b3[0])  # noqa: E731
    w_eff, w_abs = (w3 @ W2 @ W1)[0], (np.abs(w3) @ np.abs(W2) @ np.abs(W1))[0]
    off, size = job.spans()
    d = X - xb
    ys = pipe.y_std
    for k in range(len(off)):
        f = slice(off[k], off[k] + size[k])
        want = (d[:, f] * w_eff[f]).sum(1) * ys
        tol = 515 * U * (np.abs(d[:, f]) * w_abs[f]).sum(1) * ys
        assert (np.abs(out["phi_all"][k] - want) <= tol + 1e-15).all()
    e_phi = 515 * U * (np.abs(d) @ w_abs)
    bound = ys * ((X.shape[1] + 515) * U * (A(X) + A(xb)) + e_phi)
    bound = bound + 32 * 2.0 ** -53 * (np.abs(out["prediction"]) + np.abs(out["base"]) + abs(pipe.y_mean))
    print(f"steps={steps}: max |residual| {np.abs(out['residual']).max():.3e}, bound min {bound.min():.3e}")
    assert (np.abs(out["residual"]) <= bound).all()


def test_gilbert_residual_shrinks_and_a_held_column_is_zero(tmp_path):
    schema, table, *_, p = _saved(tmp_path, "gilbert")
    pred = Predictor.load(p, schema, device="cpu")
    res = [np.abs(IntegratedGradients(pred, steps=m, baseline=0).run(table)["residual"]).max() for m in (4, 8, 16, 32)]
    assert all(b < a for a, b in zip(res, res[1:])) and res[-1] < res[0] / 16  # the midpoint rule: 1 / m^2
    held = dict(table)
    held["choke"] = np.full_like(np.asarray(table["choke"], np.float32), np.float32(table["choke"][0]))
    out = IntegratedGradients(pred, steps=8, baseline=0).run(held, ["choke", "whp"])
    assert out["columns"] == ["whp", "choke"] and (out["phi"][1] == 0.0).all() and np.abs(out["phi"][0]).max() > 0


@pytest.mark.parametrize("model,extra,msg", [
    ("lstm", ["--method", "ig"], "do not apply to lstm"),
    ("cnn", ["--method", "ig"], "do not apply to cnn"),
    ("mlp", ["--method", "ig", "--repeats", "4"], "--repeats does not apply to --method ig"),
    ("mlp", ["--method", "ig", "--rep", "4"], "--repeats does not apply to --method ig"),  # an argparse abbreviation
    ("mlp", ["--method", "ig", "--seed=3"], "--seed does not apply to --method ig"),
    ("mlp", ["--steps", "8"], "--steps does not apply to --method shapley"),
    ("mlp", ["--base", "mean"], "--baseline does not apply to --method shapley"),
    ("mlp", ["--method", "ig", "--baseline", "102", "--device", "cpu"], "baseline row 102 is out of range"),
])
def test_cli_refusals(tmp_path, model, extra, msg):
    schema, table, *_ = _saved(tmp_path)
    path = str(tmp_path / "data.csv")
    write_csv(table, path, columns=NAMES.split(","))
    with pytest.raises(ValueError, match=msg):
        run_explain(model, [NAMES, TYPES, "flow", str(tmp_path) + "/", path, *extra], log=lambda *a, **k: None)
