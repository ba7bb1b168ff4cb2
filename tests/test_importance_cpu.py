"""Permutation importance on the CPU (fp32 oracle engines): the rule against a direct numpy float64
computation, the exact zeros, seeding, the per-family semantics and the job's CSV / stdout contract
(wellflow/importance.py)."""
import csv
import os

import numpy as np
import pytest
import torch

from wellflow.data.features import FeaturePipeline, take, window_starts
from wellflow.data.io import load_table, write_csv
from wellflow.data.schema import parse_schema
from wellflow.models import registry
from wellflow.utils.checkpoint import save_mdl

NAMES = "well,field,t,whp,choke,glr,temp,water_cut,dsp,flow"
TYPES = "string,string,int,float,float,float,float,float,float,float"
INPUTS = ["well", "field", "t", "whp", "choke", "glr", "temp", "water_cut", "dsp"]
QUIET = dict(log=lambda *a, **k: None)
CPU = ["--device", "cpu", "--precision", "fp32"]


def _schema():
    return parse_schema(NAMES, TYPES)


def _synth(wells, steps, seed=3):
    return load_table("synth", _schema(), synth_wells=wells, synth_steps=steps, seed=seed)


def _csv_file(dirpath, table, name="data.csv", order=None):
    t = table if order is None else take(table, order)
    t = {k: (np.asarray(v, dtype=object) if np.asarray(v).dtype.kind in "OU" else np.asarray(v)) for k, v in t.items()}
    path = os.path.join(str(dirpath), name)
    write_csv(t, path, columns=NAMES.split(","))
    return path, load_table(path, _schema())  # what the job will parse


def _read(path):
    with open(path, newline="") as f:
        rows = list(csv.reader(f))
    return rows[0], rows[1:]


def _mse(p, y, y_scale=1.0, y_shift=0.0):
    d = np.asarray(p).astype(np.float64) * y_scale + y_shift - np.asarray(y, np.float32).astype(np.float64)
    return float(np.sum(d * d)) / len(d), float(np.sum(np.abs(d))) / len(d)


@pytest.fixture(scope="module")
def mlp(tmp_path_factory):
    """An MLP with hand-set weights on the synthetic table (8 wells x 125 steps, F = 18): the
    first layer ignores the 'field' one-hot block (columns 8 .. 10) and the continuous 'temp'."""
    from wellflow.models.mlp import MLPRegressor

    d = tmp_path_factory.mktemp("imp_mlp")
    schema = _schema()
    path, table = _csv_file(d, _synth(8, 125))
    pipe = FeaturePipeline(schema, "flow", standardize_target=True).fit(table)
    assert pipe.n_features == 18 and [ix.column for ix in pipe.indexers] == ["well", "field"]
    assert pipe.block_spec()[0].tolist() == [0, 8] and pipe.continuous.index("temp") == 4
    torch.manual_seed(0)
    ref = MLPRegressor(18, (32, 16))
    with torch.no_grad():
        ref.linears()[0].weight[:, 8:11] = 0.0
        ref.linears()[0].weight[:, 11 + 4] = 0.0
    sp = str(d) + "/"
    save_mdl(sp + "models/mlp.mdl", "mlp", registry.keras_layers("mlp", ref), {"features": pipe.state()})
    ref.eval()
    return dict(sp=sp, path=path, table=table, pipe=pipe, ref=ref, schema=schema)


def _load(m, name="mlp", **kw):
    from wellflow.predict import Predictor

    return Predictor.load(m["sp"] + f"models/{name}.mdl", m["schema"], device="cpu", precision="fp32", **kw)


# ------------------------------------------------------------------ 1. the rule
def test_mlp_rule_equals_direct_numpy(mlp):
    from wellflow.importance import PermutationImportance

    table, pipe, ref = mlp["table"], mlp["pipe"], mlp["ref"]
    n, R = 1000, 2
    rng = np.random.default_rng(5)
    perms = np.stack([np.stack([rng.permutation(n) for _ in range(R)]) for _ in INPUTS])
    res = PermutationImportance(_load(mlp), repeats=R, seed=1).run(table, perms=torch.from_numpy(perms))
    assert res["scored"] == n and res["rows"] == n and not res["native"] and res["sums"].shape == (1 + 9 * R, 2)
    y = pipe.target_values(table, raw=True)

    def direct(tab):
        with torch.no_grad():
            p = ref(torch.from_numpy(pipe.features(tab))).numpy()
        assert p.dtype == np.float32
        return _mse(p, y, pipe.y_std, pipe.y_mean)

    base = direct(table)
    assert np.isclose(res["baseline_mse"], base[0], rtol=1e-10, atol=0)
    assert np.isclose(res["baseline_mae"], base[1], rtol=1e-10, atol=0)
    by = {d["column"]: d for d in res["importance"]}
    assert sorted(by) == sorted(INPUTS)
    for i, c in enumerate(INPUTS):
        want = []
        for r in range(R):
            t2 = dict(table)
            t2[c] = np.asarray(table[c])[perms[i, r]]
            want.append(direct(t2))
        got = by[c]
        assert np.allclose(got["permuted_mse"], [w[0] for w in want], rtol=1e-10, atol=0), c
        assert np.isclose(got["permuted_mse_mean"], np.mean([w[0] for w in want]), rtol=1e-10, atol=0)
        assert np.isclose(got["permuted_mae_mean"], np.mean([w[1] for w in want]), rtol=1e-10, atol=0)
        assert np.isclose(got["importance"], got["permuted_mse_mean"] - got["baseline_mse"], rtol=1e-9,
                          atol=1e-12 * got["baseline_mse"])
        assert got["kind"] == ("categorical" if c in ("well", "field") else "continuous")
        assert got["baseline_mse"] == res["baseline_mse"]
    # a column the first layer does not read: exactly zero, for a one-hot block and a continuous column
    assert by["field"]["importance"] == 0.0 and by["temp"]["importance"] == 0.0
    assert by["field"]["permuted_mse_std"] == 0.0 and by["temp"]["ratio"] == 1.0
    assert by["whp"]["importance"] > 0 and by["well"]["importance"] != 0.0
    # sorted by importance, descending
    imp = [d["importance"] for d in res["importance"]]
    assert imp == sorted(imp, reverse=True)


def test_identity_permutation_is_exactly_zero(mlp):
    from wellflow.importance import PermutationImportance

    job = PermutationImportance(_load(mlp), repeats=3)
    res = job.run(mlp["table"], perms=lambda col, r: torch.arange(1000))
    assert len(res["importance"]) == 9
    for d in res["importance"]:
        assert d["importance"] == 0.0 and d["permuted_mse"] == [res["baseline_mse"]] * 3, d
    with pytest.raises(ValueError, match=r"\[2\]\[3\]\[1000\]"):
        job.run(mlp["table"], columns=["whp", "glr"], perms=torch.zeros(2, 3, 999, dtype=torch.int64))


# ------------------------------------------------------------------ 2. the job: seed, CSV, --columns
def test_job_seed_csv_schema_and_columns(mlp, tmp_path):
    from wellflow.importance import CSV_COLUMNS, run_importance

    sp, path = mlp["sp"], mlp["path"]
    args = ["mlp", [NAMES, TYPES, "flow", sp, path, *CPU, "--repeats", "3"]]
    lines = []
    a = run_importance(args[0], args[1] + ["--seed", "7"], log=lambda s: lines.append(str(s)))
    assert a["out"] == sp + "importance/mlp.csv" and not os.path.exists(a["out"] + ".tmp")
    with open(a["out"], "rb") as f:
        first = f.read()
    b = run_importance(args[0], args[1] + ["--seed", "7", "--out", str(tmp_path / "again.csv")], **QUIET)
    with open(tmp_path / "again.csv", "rb") as f:
        assert f.read() == first
    c = run_importance(args[0], args[1] + ["--seed", "8", "--out", str(tmp_path / "other.csv")], **QUIET)
    assert c["baseline_mse"] == a["baseline_mse"] == b["baseline_mse"]
    ca, cc = ({d["column"]: d for d in r["importance"]} for r in (a, c))
    assert ca["whp"]["permuted_mse"] != cc["whp"]["permuted_mse"]
    assert cc["field"]["importance"] == 0.0  # ... whatever the shuffle

    head, rows = _read(a["out"])
    assert tuple(head) == CSV_COLUMNS == ("column", "kind", "baseline_mse", "permuted_mse_mean", "permuted_mse_std",
                                          "importance", "ratio", "baseline_mae", "permuted_mae_mean")
    assert len(rows) == 9 and sorted(r[0] for r in rows) == sorted(INPUTS)
    assert [r[0] for r in rows] == [d["column"] for d in a["importance"]]
    imp = [float(r[5]) for r in rows]
    assert imp == sorted(imp, reverse=True) and imp[0] > 0
    for r, d in zip(rows, a["importance"]):
        assert r[1] == d["kind"] and float(r[2]) == a["baseline_mse"] and float(r[7]) == a["baseline_mae"]
        assert float(r[3]) == d["permuted_mse_mean"] and float(r[4]) == d["permuted_mse_std"]
        assert float(r[5]) == d["importance"] and float(r[8]) == d["permuted_mae_mean"]
        assert np.isclose(float(r[6]), float(r[3]) / float(r[2]), rtol=1e-12)
    assert lines[0] == "Rows scored: 1000" and lines[1] == "Baseline MSE: %f" % a["baseline_mse"]
    assert len(lines) == 11 and [l.split(" ")[0] for l in lines[2:]] == [r[0] for r in rows]

    s = run_importance(args[0], args[1] + ["--columns", "choke,well", "--out", str(tmp_path / "sub.csv")], **QUIET)
    head, rows = _read(str(tmp_path / "sub.csv"))
    assert sorted(r[0] for r in rows) == ["choke", "well"] and len(s["importance"]) == 2
    assert s["sums"].shape == (1 + 2 * 3, 2) and s["baseline_mse"] == a["baseline_mse"]


def test_submit_dispatches_importance(tmp_path, capsys):
    from wellflow import submit
    from wellflow.train.job import run_job

    sp = str(tmp_path) + "/"
    run_job("gilbert", [NAMES, TYPES, "flow", sp, "--synth-wells", "2", "--synth-steps", "50"], **QUIET)
    path, table = _csv_file(tmp_path, _synth(2, 50))
    assert submit.main(["importance", "gilbert", NAMES, TYPES, "flow", sp, path, "--repeats", "2"]) == 0
    out = capsys.readouterr().out
    assert "Rows scored: 100" in out and "Baseline MSE: " in out
    head, rows = _read(sp + "importance/gilbert.csv")
    assert head[0] == "column" and sorted(r[0] for r in rows) == ["choke", "glr", "whp"]


# ------------------------------------------------------------------ 3. LSTM
def test_lstm_windows_of_interleaved_series(tmp_path):
    from wellflow.importance import PermutationImportance
    from wellflow.models.lstm import LSTMRegressor
    from wellflow.predict import Predictor

    T, H = 8, 16
    schema = _schema()
    base = _synth(3, 40)
    inter = np.arange(120).reshape(3, 40).T.ravel()  # t0 of every well, t1 of every well, ...
    _, table = _csv_file(tmp_path, base, order=inter)
    assert list(table["well"][:4]) == ["W000", "W001", "W002", "W000"]
    pipe = FeaturePipeline(schema, "flow").fit(table)  # target left raw: predictions are network outputs
    torch.manual_seed(2)
    ref = LSTMRegressor(pipe.n_features, H)
    p = str(tmp_path / "models" / "lstm.mdl")
    save_mdl(p, "lstm", registry.keras_layers("lstm", ref),
             {"features": pipe.state(), "job": {"seq_len": T, "group_col": "well", "hidden": H}})
    pred = Predictor.load(p, schema, device="cpu", precision="fp32")
    n, R = 120, 2
    rng = np.random.default_rng(9)
    perms = np.stack([np.stack([rng.permutation(n) for _ in range(R)])])
    res = PermutationImportance(pred, repeats=R).run(table, columns=["choke"], perms=perms)
    assert res["rows"] == 120 and res["scored"] == 3 * (40 - T + 1) == 99
    y = pipe.target_values(table, raw=True)
    out = pred.predict_table(table)  # standardised == raw here: the target is not standardised
    ok = ~np.isnan(out)
    assert ok.sum() == 99
    assert np.isclose(res["baseline_mse"], _mse(out[ok], y[ok])[0], rtol=1e-10, atol=0)
    # the permutation acts on the series-sorted table; a window's target is its last row's
    ids = np.unique(np.asarray(table["well"]).astype(str), return_inverse=True)[1]
    order = np.argsort(ids, kind="stable")
    stable = take(table, order)
    starts = np.asarray(window_starts(n, T, ids[order]))
    ref.eval()
    for r in range(R):
        t2 = dict(stable)
        t2["choke"] = np.asarray(stable["choke"])[perms[0, r]]
        X = pipe.features(t2)
        with torch.no_grad():
            pw = ref(torch.from_numpy(X[starts[:, None] + np.arange(T)[None, :]])).numpy()
        want = _mse(pw, y[order][starts + T - 1])[0]
        assert np.isclose(res["importance"][0]["permuted_mse"][r], want, rtol=1e-6, atol=0)
    # every series shorter than the window: nothing to score, said so
    with pytest.raises(ValueError, match="shorter than the window"):
        PermutationImportance(pred).run(take(table, np.arange(15)))


# ------------------------------------------------------------------ 4. Gilbert
def test_gilbert_on_its_own_output(tmp_path):
    from wellflow.importance import PermutationImportance
    from wellflow.models.gilbert import GilbertModel
    from wellflow.predict import Predictor

    table = dict(_synth(2, 60))
    table["flow"] = GilbertModel(correlation="ros").predict(
        {k: np.asarray(table[k], np.float64) for k in ("whp", "choke", "glr")})
    p = str(tmp_path / "models" / "gilbert.mdl")
    save_mdl(p, "gilbert", [("Gilbert", [torch.tensor([17.4, 0.5, 2.0])])], {"correlation": "ros", "glr_unit": "scf"})
    job = PermutationImportance(Predictor.load(p, _schema(), device="cpu"), repeats=4, seed=3)
    res = job.run(table, target="flow")
    assert res["baseline_mse"] == 0.0 and res["baseline_mae"] == 0.0 and res["scored"] == 120
    assert sorted(d["column"] for d in res["importance"]) == ["choke", "glr", "whp"]
    assert all(d["importance"] > 0 and d["kind"] == "continuous" for d in res["importance"])
    with pytest.raises(ValueError, match="whp, choke, glr"):
        job.run(table, columns=["temp"], target="flow")


# ------------------------------------------------------------------ 5. refusals
def test_cnn_is_refused_with_the_reason(tmp_path):
    from wellflow.importance import run_importance
    from wellflow.models.cnn import CNN1DRegressor

    schema = _schema()
    path, table = _csv_file(tmp_path, _synth(2, 100))
    pipe = FeaturePipeline(schema, "flow", standardize_target=True).fit(table)
    ref = CNN1DRegressor(48, 1, 100, 13, 12).init_keras(5)
    sp = str(tmp_path) + "/"
    save_mdl(sp + "models/cnn.mdl", "cnn", registry.keras_layers("cnn", ref), {"features": pipe.state()})
    with pytest.raises(ValueError, match="target's own history.*no input column to permute"):
        run_importance("cnn", [NAMES, TYPES, "flow", sp, path, *CPU], **QUIET)
    assert not os.path.exists(sp + "importance/cnn.csv")


def test_errors_name_the_cause(mlp, tmp_path):
    from wellflow.importance import PermutationImportance, run_importance

    table = mlp["table"]
    job = PermutationImportance(_load(mlp), repeats=1)
    no_target = {k: v for k, v in table.items() if k != "flow"}
    with pytest.raises(ValueError, match="lacks the target column 'flow'"):
        job.run(no_target)
    words = dict(table)
    words["flow"] = np.asarray(["high"] * 1000, dtype=object)
    with pytest.raises(ValueError, match="'flow' is not numeric"):
        job.run(words)
    with pytest.raises(ValueError, match="unknown column 'nope'"):
        job.run(table, columns=["nope"])
    with pytest.raises(ValueError, match="unknown column 'flow'"):  # the target is no input
        run_importance("mlp", [NAMES, TYPES, "flow", mlp["sp"], mlp["path"], *CPU, "--columns", "flow"], **QUIET)
    with pytest.raises(ValueError, match="repeats"):
        PermutationImportance(_load(mlp), repeats=0)
    # a .mdl that no training job wrote: no pipeline state
    sp = str(tmp_path) + "/"
    save_mdl(sp + "models/mlp.mdl", "mlp", registry.keras_layers("mlp", mlp["ref"]), {"epoch": 1})
    with pytest.raises(ValueError, match="features"):
        run_importance("mlp", [NAMES, TYPES, "flow", sp, mlp["path"], *CPU], **QUIET)
    with pytest.raises(FileNotFoundError, match="lstm.mdl"):
        run_importance("lstm", [NAMES, TYPES, "flow", sp, mlp["path"], *CPU], **QUIET)
