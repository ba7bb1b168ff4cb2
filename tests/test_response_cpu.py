"""Response curves on the CPU (fp32 oracle engines): the rule against a direct numpy float64
computation, the exact zeros, the grids, the per-family semantics and the job's CSV / stdout contract
(wellflow/response.py)."""
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
QUIET = dict(log=lambda *a, **k: None)
CPU = ["--device", "cpu", "--precision", "fp32"]
HEADER = ("column", "kind", "value", "group", "rows", "mean_prediction", "std_prediction", "delta")


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


def _bincount(v, ids, G):
    v = np.asarray(v, np.float64)
    return np.stack([np.bincount(ids, minlength=G).astype(np.float64), np.bincount(ids, weights=v, minlength=G),
                     np.bincount(ids, weights=v * v, minlength=G)], axis=1)


def _replaced(table, col, value):
    t = dict(table)
    n = len(table[col])
    t[col] = np.full(n, value, object) if isinstance(value, str) else np.full(n, value, np.float32)
    return t


@pytest.fixture(scope="module")
def mlp(tmp_path_factory):
    """An MLP with hand-set weights on the synthetic table (8 wells x 125 steps, F = 18): the
    first layer ignores the 'field' one-hot block (columns 8 .. 10) and the continuous 'temp'."""
    from wellflow.models.mlp import MLPRegressor

    d = tmp_path_factory.mktemp("resp_mlp")
    schema = _schema()
    path, table = _csv_file(d, _synth(8, 125))
    pipe = FeaturePipeline(schema, "flow", standardize_target=True).fit(table)
    assert pipe.n_features == 18 and [ix.column for ix in pipe.indexers] == ["well", "field"]
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
    from wellflow.response import ResponseCurves

    table, pipe, ref = mlp["table"], mlp["pipe"], mlp["ref"]
    grid = [0.5, 0.1, 0.9]  # kept in the order given
    notes = []
    res = ResponseCurves(_load(mlp), note=notes.append).run(
        table, ["choke", "well"], grids={"choke": grid, "well": ["W003", "nowhere", "W000"]}, by="well")
    assert res["scored"] == 1000 and res["rows"] == 1000 and not res["native"]
    groups, ids = np.unique(np.asarray(table["well"]).astype(str), return_inverse=True)
    assert res["groups"] == list(groups) and len(groups) == 8 and res["sums"].shape == (1 + 3 + 3, 8, 3)
    assert res["grids"]["choke"] == [repr(float(np.float32(v))) for v in grid]
    assert res["grids"]["well"] == ["W003", "nowhere", "W000"]
    assert len(notes) == 1 and "nowhere" in notes[0] and "unknown index" in notes[0]  # accepted, noted once

    def direct(tab):
        with torch.no_grad():
            p = ref(torch.from_numpy(pipe.features(tab))).numpy()
        assert p.dtype == np.float32
        return _bincount(p.astype(np.float64) * pipe.y_std + pipe.y_mean, ids, 8)

    want = [direct(table)] + [direct(_replaced(table, "choke", np.float32(v))) for v in grid] + \
           [direct(_replaced(table, "well", v)) for v in ("W003", "nowhere", "W000")]
    assert np.allclose(res["sums"], np.asarray(want), rtol=1e-10, atol=0)
    assert (res["sums"][:, :, 0] == 125).all()
    # the unseen label maps to the unknown index, which lies outside the kept one-hot columns
    X = pipe.features(_replaced(table, "well", "nowhere"))
    assert (X[:, :8].sum(axis=1) == 0).all()
    # the cells: mean / std / delta from the sums; overall = the groups' sums in group order
    cur = res["curves"]
    assert len(cur) == 7 * 9
    s = res["sums"]
    for slot in range(7):
        blk = cur[slot * 9 : slot * 9 + 9]
        assert [d["group"] for d in blk] == [""] + list(groups)
        tot = np.cumsum(s[slot], axis=0)[-1]
        btot = np.cumsum(s[0], axis=0)[-1]
        assert blk[0]["rows"] == 1000 and blk[0]["mean_prediction"] == tot[1] / tot[0]
        assert blk[0]["delta"] == tot[1] / tot[0] - btot[1] / btot[0]
        for i, d in enumerate(blk[1:]):
            mean = s[slot, i, 1] / 125
            assert d["rows"] == 125 and d["mean_prediction"] == mean
            assert d["std_prediction"] == np.sqrt(max(0.0, s[slot, i, 2] / 125 - mean * mean))
            assert d["delta"] == mean - s[0, i, 1] / 125
    assert all(d["delta"] == 0.0 and d["kind"] == "baseline" and d["column"] == "" and d["value"] == "" for d in cur[:9])
    assert [d["kind"] for d in cur[9::9]] == ["continuous"] * 3 + ["categorical"] * 3
    assert any(d["delta"] != 0.0 for d in cur[9:])


def test_unused_columns_give_exact_zeros(mlp):
    from wellflow.response import ResponseCurves

    res = ResponseCurves(_load(mlp), points=3).run(mlp["table"], ["field", "temp"], by="well")
    assert res["sums"].shape[0] == 1 + 3 + 3
    for slot in range(1, 7):
        assert np.array_equal(res["sums"][slot], res["sums"][0])  # bit for bit
    assert all(d["delta"] == 0.0 for d in res["curves"])


def test_default_and_explicit_grids(mlp):
    from wellflow.response import ResponseCurves

    table, pipe = mlp["table"], mlp["pipe"]
    res = ResponseCurves(_load(mlp), points=5).run(table, ["whp", "field", "t"])
    col = np.asarray(table["whp"], np.float32)
    want = np.linspace(float(col.min()), float(col.max()), 5, dtype=np.float64).astype(np.float32)
    assert res["grids"]["whp"] == [repr(float(v)) for v in want]
    field = next(ix for ix in pipe.indexers if ix.column == "field")
    assert res["grids"]["field"] == list(field.labels) and len(field.labels) == 3  # indexer order
    t = np.asarray(table["t"], np.float32)  # an int column is a continuous source
    assert res["grids"]["t"][0] == repr(float(t.min())) and res["grids"]["t"][-1] == repr(float(t.max()))
    # without --by: one group, only the overall cells
    assert res["groups"] == [] and res["sums"].shape == (1 + 5 + 3 + 5, 1, 3) and len(res["curves"]) == 14
    assert all(d["group"] == "" and d["rows"] == 1000 for d in res["curves"])
    assert [d["column"] for d in res["curves"]] == [""] + ["whp"] * 5 + ["field"] * 3 + ["t"] * 5
    nine = ResponseCurves(_load(mlp)).run(table, ["whp"])  # --points defaults to 9
    assert len(nine["grids"]["whp"]) == 9
    exp = ResponseCurves(_load(mlp)).run(table, ["choke"], grids={"choke": ["0.75", 0.25, 0.5]})
    assert exp["grids"]["choke"] == ["0.75", "0.25", "0.5"] and [d["value"] for d in exp["curves"][1:]] == ["0.75", "0.25", "0.5"]


# ------------------------------------------------------------------ 2. the job: CSV, stdout, dispatch, ranks
def test_job_csv_layout_and_stdout(mlp, tmp_path):
    from wellflow.response import CSV_COLUMNS, run_response

    sp, path = mlp["sp"], mlp["path"]
    lines = []
    res = run_response("mlp", [NAMES, TYPES, "flow", sp, path, *CPU, "--columns", "choke,field", "--points", "4",
                               "--by", "well"], log=lambda s: lines.append(str(s)))
    assert res["out"] == sp + "response/mlp.csv" and not os.path.exists(res["out"] + ".tmp")
    head, rows = _read(res["out"])
    assert tuple(head) == CSV_COLUMNS == HEADER
    assert len(rows) == (1 + 4 + 3) * (1 + 8)
    wells = sorted(set(np.asarray(mlp["table"]["well"]).astype(str)))
    for b in range(8):
        blk = rows[b * 9 : b * 9 + 9]
        assert [r[3] for r in blk] == [""] + wells                      # overall, then the groups
        assert [int(r[4]) for r in blk] == [1000] + [125] * 8
        assert len({(r[0], r[1], r[2]) for r in blk}) == 1
    assert [rows[b * 9][0] for b in range(8)] == [""] + ["choke"] * 4 + ["field"] * 3
    assert [rows[b * 9][1] for b in range(8)] == ["baseline"] + ["continuous"] * 4 + ["categorical"] * 3
    assert [rows[b * 9][2] for b in range(8)] == [""] + res["grids"]["choke"] + res["grids"]["field"]
    for r, d in zip(rows, res["curves"]):
        assert float(r[5]) == d["mean_prediction"] and float(r[6]) == d["std_prediction"] and float(r[7]) == d["delta"]
        assert r[5] == repr(d["mean_prediction"])
    assert all(float(r[7]) == 0.0 for r in rows[:9]) and all(float(r[7]) == 0.0 for r in rows[5 * 9 :])  # field: unused
    assert lines[0] == "Rows scored: 1000" and lines[1] == "Baseline mean prediction: %f" % res["baseline_mean"]
    assert len(lines) == 2 + 4 + 3 and lines[2].startswith("choke = " + res["grids"]["choke"][0] + ":")
    assert {"model", "native", "rows", "scored", "groups", "grids", "sums", "curves"} <= set(res)
    # --out, --grid
    out2 = str(tmp_path / "deep" / "curve.csv")
    g = run_response("mlp", [NAMES, TYPES, "flow", sp, path, *CPU, "--columns", "choke", "--grid", "0.3,0.2", "--out", out2],
                     **QUIET)
    head, rows = _read(out2)
    assert g["out"] == out2 and [r[2] for r in rows] == ["", repr(float(np.float32(0.3))), repr(float(np.float32(0.2)))]


def test_submit_dispatches_response(tmp_path, capsys):
    from wellflow import submit
    from wellflow.train.job import run_job

    sp = str(tmp_path) + "/"
    run_job("gilbert", [NAMES, TYPES, "flow", sp, "--synth-wells", "2", "--synth-steps", "50"], **QUIET)
    path, table = _csv_file(tmp_path, _synth(2, 50))
    assert submit.main(["response", "gilbert", NAMES, TYPES, "flow", sp, path, "--columns", "choke", "--points", "3"]) == 0
    out = capsys.readouterr().out
    assert "Rows scored: 100" in out and "Baseline mean prediction: " in out
    head, rows = _read(sp + "response/gilbert.csv")
    assert tuple(head) == HEADER and [r[0] for r in rows] == ["", "choke", "choke", "choke"]


def test_other_ranks_skip(mlp, tmp_path, monkeypatch):
    from wellflow.response import run_response

    monkeypatch.setenv("RANK", "1")
    out = str(tmp_path / "r1.csv")
    res = run_response("mlp", [NAMES, TYPES, "flow", mlp["sp"], mlp["path"], *CPU, "--columns", "choke", "--out", out], **QUIET)
    assert res.get("skipped") is True and not os.path.exists(out)


# ------------------------------------------------------------------ 3. LSTM
def test_lstm_windows_of_interleaved_series(tmp_path):
    from wellflow.models.lstm import LSTMRegressor
    from wellflow.predict import Predictor
    from wellflow.response import ResponseCurves

    T, H = 8, 16
    schema = _schema()
    base = _synth(3, 40)
    inter = np.arange(120).reshape(3, 40).T.ravel()  # t0 of every well, t1 of every well, ...
    # W002 is cut to 5 rows (shorter than the window): a group without a prediction
    keep = np.asarray([i for i in inter if not (i // 40 == 2 and i % 40 >= 5)])
    _, table = _csv_file(tmp_path, base, order=keep)
    n = len(table["well"])
    assert n == 85 and list(table["well"][:4]) == ["W000", "W001", "W002", "W000"]
    pipe = FeaturePipeline(schema, "flow").fit(table)  # target left raw: predictions are network outputs
    torch.manual_seed(2)
    ref = LSTMRegressor(pipe.n_features, H)
    p = str(tmp_path / "models" / "lstm.mdl")
    save_mdl(p, "lstm", registry.keras_layers("lstm", ref),
             {"features": pipe.state(), "job": {"seq_len": T, "group_col": "well", "hidden": H}})
    pred = Predictor.load(p, schema, device="cpu", precision="fp32")
    grid = [0.2, 0.8]
    res = ResponseCurves(pred).run(table, ["choke"], grids={"choke": grid}, by="well")
    assert res["rows"] == 85 and res["scored"] == 2 * (40 - T + 1) == 66 and res["groups"] == ["W000", "W001", "W002"]
    # a window belongs to the group of its last row; the column is constant over all timesteps
    ids = np.unique(np.asarray(table["well"]).astype(str), return_inverse=True)[1]
    order = np.argsort(ids, kind="stable")
    stable = take(table, order)
    starts = np.asarray(window_starts(n, T, ids[order]))
    wid = ids[order][starts + T - 1]
    ref.eval()
    want = []
    for v in [None] + grid:
        t2 = stable if v is None else _replaced(stable, "choke", np.float32(v))
        X = pipe.features(t2)
        Xw = X[starts[:, None] + np.arange(T)[None, :]]
        if v is not None:
            k = pipe.n_features - len(pipe.continuous) + pipe.continuous.index("choke")
            assert (Xw[:, :, k] == Xw[0, 0, k]).all()
        with torch.no_grad():
            want.append(_bincount(ref(torch.from_numpy(Xw)).numpy(), wid, 3))
    assert np.allclose(res["sums"], np.asarray(want), rtol=1e-6, atol=0)
    assert res["sums"][:, :, 0].tolist() == [[33.0, 33.0, 0.0]] * 3
    # 'rows' per cell; the empty group's cells are empty
    blk = res["curves"][4:8]
    assert [d["rows"] for d in blk] == [66, 33, 33, 0]
    assert blk[3]["mean_prediction"] is None and blk[3]["delta"] is None and blk[3]["std_prediction"] is None
    from wellflow.response import _write_csv

    _write_csv(str(tmp_path / "l.csv"), res["curves"])
    head, rows = _read(str(tmp_path / "l.csv"))
    assert rows[7][3:] == ["W002", "0", "", "", ""]
    # every series shorter than the window: nothing to score, said so
    with pytest.raises(ValueError, match="shorter than the window"):
        ResponseCurves(pred).run(take(table, np.arange(15)), ["choke"])


# ------------------------------------------------------------------ 4. Gilbert
def test_gilbert_curve_over_choke(tmp_path):
    from wellflow.models.gilbert import GilbertModel
    from wellflow.predict import Predictor
    from wellflow.response import ResponseCurves

    table = dict(_synth(2, 60))
    p = str(tmp_path / "models" / "gilbert.mdl")
    save_mdl(p, "gilbert", [("Gilbert", [torch.tensor([17.4, 0.5, 2.0])])], {"correlation": "ros", "glr_unit": "scf"})
    job = ResponseCurves(Predictor.load(p, _schema(), device="cpu"), points=4)
    res = job.run(table, ["choke"], by="well")
    assert res["scored"] == 120 and not res["native"] and res["sums"].shape == (5, 2, 3)
    ids = np.unique(np.asarray(table["well"]).astype(str), return_inverse=True)[1]
    cols = {k: np.asarray(table[k], np.float64) for k in ("whp", "choke", "glr")}
    model = GilbertModel(correlation="ros")
    col = np.asarray(table["choke"], np.float32)
    grid = np.linspace(float(col.min()), float(col.max()), 4, dtype=np.float64).astype(np.float32)
    want = [_bincount(model.predict(cols), ids, 2)]
    for v in grid:
        c2 = dict(cols)
        c2["choke"] = np.full(120, v, np.float64)
        want.append(_bincount(model.predict(c2), ids, 2))
    assert np.array_equal(res["sums"], np.asarray(want))  # exactly
    means = [d["mean_prediction"] for d in res["curves"][3::3]]
    assert means == sorted(means) and means[0] < means[-1]  # flow grows with the choke size
    with pytest.raises(ValueError, match="unknown column 'temp': gilbert reads only whp, choke, glr"):
        job.run(table, ["temp"])


# ------------------------------------------------------------------ 5. refusals
def test_cnn_is_refused_with_the_reason(tmp_path):
    from wellflow.models.cnn import CNN1DRegressor
    from wellflow.response import run_response

    schema = _schema()
    path, table = _csv_file(tmp_path, _synth(2, 100))
    pipe = FeaturePipeline(schema, "flow", standardize_target=True).fit(table)
    ref = CNN1DRegressor(48, 1, 100, 13, 12).init_keras(5)
    sp = str(tmp_path) + "/"
    save_mdl(sp + "models/cnn.mdl", "cnn", registry.keras_layers("cnn", ref), {"features": pipe.state()})
    with pytest.raises(ValueError, match="target's own history.*no input column"):
        run_response("cnn", [NAMES, TYPES, "flow", sp, path, *CPU, "--columns", "choke"], **QUIET)
    assert not os.path.exists(sp + "response/cnn.csv")


def test_errors_name_the_cause(mlp, tmp_path):
    from wellflow.response import ResponseCurves, run_response

    table = mlp["table"]
    job = ResponseCurves(_load(mlp))
    args = [NAMES, TYPES, "flow", mlp["sp"], mlp["path"], *CPU]
    with pytest.raises(ValueError, match="unknown column 'nope'"):
        job.run(table, ["nope"])
    with pytest.raises(ValueError, match="'flow' is the target column"):
        run_response("mlp", args + ["--columns", "flow"], **QUIET)
    with pytest.raises(ValueError, match="no column to sweep.*--columns"):
        run_response("mlp", args, **QUIET)
    with pytest.raises(ValueError, match="no column to sweep"):
        run_response("mlp", args + ["--columns", " , "], **QUIET)
    with pytest.raises(ValueError, match="no column to sweep"):
        job.run(table, [])
    with pytest.raises(ValueError, match="column 'choke' listed twice"):
        run_response("mlp", args + ["--columns", "choke,whp,choke"], **QUIET)
    with pytest.raises(ValueError, match="points must be >= 2"):
        run_response("mlp", args + ["--columns", "choke", "--points", "1"], **QUIET)
    with pytest.raises(ValueError, match="grid value 'wide' of the continuous column 'choke' is not a number"):
        run_response("mlp", args + ["--columns", "choke", "--grid", "0.5,wide"], **QUIET)
    with pytest.raises(ValueError, match="--grid gives ONE column's values; 2 columns"):
        run_response("mlp", args + ["--columns", "choke,whp", "--grid", "0.5"], **QUIET)
    with pytest.raises(ValueError, match="lacks the --by column 'pad'"):
        run_response("mlp", args + ["--columns", "choke", "--by", "pad"], **QUIET)
    big = {k: np.tile(np.asarray(v), 17) for k, v in table.items()}
    big["t"] = np.arange(17000)  # 17000 distinct values > the cap of 16384 groups
    with pytest.raises(ValueError, match="17000 groups; at most 16384"):
        job.run(big, ["choke"], by="t")
    with pytest.raises(ValueError, match="no rows to score"):
        job.run({k: np.asarray(v)[:0] for k, v in table.items()}, ["choke"])
    with pytest.raises(ValueError, match="lacks the input column 'glr'"):
        job.run({k: v for k, v in table.items() if k != "glr"}, ["choke"])
