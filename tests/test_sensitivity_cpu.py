"""The sensitivity job on the CPU (wellflow/sensitivity.py): Gilbert's constant elasticities, the
oracle route against float64 on the exact lattice, every refusal and the job's CSV and notices."""
import csv

import numpy as np
import pytest
import torch

from wellflow.data.features import FeaturePipeline
from wellflow.data.io import load_table, write_csv
from wellflow.data.schema import parse_schema
from wellflow.models import registry
from wellflow.models.mlp import MlpLayout, MLPRegressor
from wellflow.predict import Predictor
from wellflow.sensitivity import Sensitivity, run_sensitivity
from wellflow.utils.checkpoint import save_mdl

NAMES = "well,field,t,whp,choke,glr,temp,water_cut,dsp,flow"
TYPES = "string,string,int,float,float,float,float,float,float,float"
HID = (256, 256)


def _saved(tmp_path, name="mlp", wells=3):
    """(schema, table, pipe, reference model, path of the saved .mdl) of a model planted on the synthetic table."""
    schema = parse_schema(NAMES, TYPES)
    table = load_table("synth", schema, synth_wells=wells, synth_steps=100 // wells + 1, seed=3)
    p = str(tmp_path / "models" / f"{name}.mdl")
    if name == "gilbert":
        save_mdl(p, name, [("Gilbert", [torch.tensor([17.4, 0.5, 2.0])])], {"correlation": "ros", "glr_unit": "scf"})
        return schema, table, None, None, p
    pipe = FeaturePipeline(schema, "flow", standardize_target=True).fit(table)
    torch.manual_seed(0)
    ref = MLPRegressor(pipe.n_features, HID) if name == "mlp" else registry.build_reference(name, _cfg(name), pipe.n_features, 1)
    save_mdl(p, name, registry.keras_layers(name, ref), {"features": pipe.state()})
    return schema, table, pipe, ref, p


def _cfg(name):
    from wellflow.config import MODEL_DEFAULTS, RunConfig

    return RunConfig(model=name, **MODEL_DEFAULTS[name])


def test_gilbert_elasticities_are_the_exponents(tmp_path):
    schema, table, *_, p = _saved(tmp_path, "gilbert")
    out = Sensitivity(Predictor.load(p, schema, device="cpu")).run(table)
    assert out["columns"] == ["whp", "choke", "glr"] and not out["native"]
    for k, (c, want) in enumerate((("whp", 1.0), ("choke", 2.0), ("glr", -0.5))):  # ros: B = 0.5, C = 2
        x = np.asarray(table[c], np.float32).astype(np.float64)
        assert np.abs(out["elast"][k] - want).max() <= 4 * 2.0 ** -52 * abs(want)
        assert np.array_equal(out["grad"][k] * x / out["prediction"], out["elast"][k])


def test_oracle_route_equals_float64_on_the_lattice(tmp_path):
    from wellflow.train import exact as ex

    schema, table, pipe, ref, p = _saved(tmp_path)
    F = pipe.n_features
    assert F == 13  # 2 + 4 one-hot columns, 7 continuous
    case = ex.exact_mlp_case(F, HID, 100, 100 * F + 302)
    ((W1, b1), (W2, b2)), w3, _ = MlpLayout(F, HID).views(case.flat)
    ref.load_flat(case.flat)
    save_mdl(p, "mlp", registry.keras_layers("mlp", ref), {"features": pipe.state()})
    pred = Predictor.load(p, schema, device="cpu", precision="fp32")
    notes = []
    out = Sensitivity(pred, note=notes.append).run(table, ["glr", "whp"])
    assert out["columns"] == ["whp", "glr"] and not out["native"] and len(notes) == 1 and "oracle" in notes[0]
    x = torch.from_numpy(pipe.features(table)).double()
    z1 = x @ W1[:, :F].t() + b1
    z2 = torch.relu(z1) @ W2.t() + b2
    dx = ((z1 > 0) * (((z2 > 0) * w3) @ W2)) @ W1[:, :F]
    cont, std = list(pipe.continuous), pipe.scale()[1].astype(np.float64)
    for k, c in enumerate(out["columns"]):
        q = cont.index(c)
        g = dx[:, F - len(cont) + q].numpy()
        assert np.array_equal(g.astype(np.float32).astype(np.float64), g)  # fp32 holds the weight products
        assert np.array_equal(out["grad"][k], g * pipe.y_std / std[q])


@pytest.mark.parametrize("name,columns,msg", [
    ("lstm", None, "lstm: a gradient through the windows is not built"),
    ("cnn", None, "cnn: the CNN reads only the target's own history"),
    ("mlp", ["well"], "'well' is categorical"),
    ("mlp", ["flow"], "'flow' is the target column"),
    ("mlp", ["depth"], "unknown column 'depth'"),
    ("gilbert", ["temp"], "gilbert reads only whp, choke, glr"),
])
def test_refusals(tmp_path, name, columns, msg):
    schema, table, *_, p = _saved(tmp_path, name)
    with pytest.raises(ValueError, match=msg):
        Sensitivity(Predictor.load(p, schema, device="cpu", precision="fp32"), note=lambda s: None).run(table, columns)


def test_job_csv_and_notice_on_the_cpu(tmp_path, capsys):
    schema, table, pipe, ref, p = _saved(tmp_path)
    path = str(tmp_path / "data.csv")
    write_csv(table, path, columns=NAMES.split(","))
    lines = []
    res = run_sensitivity("mlp", [NAMES, TYPES, "flow", str(tmp_path) + "/", path, "--columns", "glr,choke", "--device", "cpu"],
                          log=lines.append)  # --precision bf16 (the default) on the CPU: the oracle, announced
    assert "oracle route" in capsys.readouterr().err and not res["native"]
    assert res["out"] == str(tmp_path) + "/sensitivity/mlp.csv" and res["columns"] == ["choke", "glr"]
    with open(res["out"], newline="") as f:
        rows = list(csv.reader(f))
    assert rows[0] == NAMES.split(",") + ["prediction", "grad_choke", "elast_choke", "grad_glr", "elast_glr"]
    back = np.asarray([[float(c) for c in r[10:]] for r in rows[1:]])
    assert len(back) == len(table["well"]) == 102 and np.array_equal(back[:, 0], res["prediction"])
    assert np.array_equal(back[:, 1::2].T, res["grad"]) and np.array_equal(back[:, 2::2].T, res["elast"])
    assert lines[0] == "Rows scored: 102" and lines[1].startswith("Mean prediction: ") and len(lines) == 4
    assert {l.split(":")[0] for l in lines[2:]} == {"choke", "glr"} and "median elast" in lines[2]
