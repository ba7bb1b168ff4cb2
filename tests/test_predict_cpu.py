"""Prediction job on the CPU (fp32 oracle engines): pipeline restore, raw-column export, the
per-family scoring semantics and the job's CSV / stdout contract (wellflow/predict.py)."""
import csv
import json
import os

import numpy as np
import pytest
import torch

from wellflow.data.features import FeaturePipeline, StringIndexer, take
from wellflow.data.io import load_table, write_csv
from wellflow.data.schema import parse_schema
from wellflow.data.synth import well_log_table
from wellflow.models import registry
from wellflow.utils.checkpoint import load_mdl, save_mdl

NAMES = "well,field,t,whp,choke,glr,temp,water_cut,dsp,flow"
TYPES = "string,string,int,float,float,float,float,float,float,float"
QUIET = dict(log=lambda *a, **k: None)


def _schema():
    return parse_schema(NAMES, TYPES)


def _synth(wells, steps, seed=42):
    return load_table("synth", _schema(), synth_wells=wells, synth_steps=steps, seed=seed)


def _read_out(path):
    with open(path, newline="") as f:
        return [row for row in csv.reader(f)]


def _pred_col(rows, k=-1):
    return np.asarray([np.nan if r[k] == "" else float(r[k]) for r in rows], np.float64)


def _assert_echo(rows, table, names):
    """The first len(names) cells of every output line are the parsed table's values."""
    assert all(len(r) >= len(names) for r in rows)
    for j, c in enumerate(names):
        v = np.asarray(table[c])
        got = [r[j] for r in rows]
        if v.dtype == object:
            assert got == [str(x) for x in v], c
        else:
            assert np.array_equal(np.asarray([float(g) for g in got]).astype(v.dtype), v), c


# ------------------------------------------------------------------ 1. from_state
def test_from_state_round_trip_and_errors():
    schema = _schema()
    table = _synth(6, 100)
    pipe = FeaturePipeline(schema, "flow", standardize_target=True).fit(take(table, np.arange(300)))
    state = json.loads(json.dumps(pipe.state()))
    back = FeaturePipeline.from_state(schema, state)
    assert "W005" not in pipe.indexers[0].labels  # the full table holds labels unseen in training
    X0, y0 = pipe.transform(table)
    X1, y1 = back.transform(table)
    assert X1.dtype == np.float32 and np.array_equal(X0, X1) and np.array_equal(y0, y1)
    assert back.n_features == pipe.n_features
    assert np.array_equal(back.inverse_target(y1), pipe.inverse_target(y0))

    with pytest.raises(ValueError, match="state"):
        FeaturePipeline.from_state(schema, None)
    for k in pipe.state():
        bad = {kk: v for kk, v in state.items() if kk != k}
        with pytest.raises(ValueError, match=k):
            FeaturePipeline.from_state(schema, bad)
    # the schema types 'field' as a number: the saved categorical column is not one of the schema's
    other = parse_schema(NAMES, TYPES.replace("string,string", "string,float", 1))
    with pytest.raises(ValueError, match="'field'"):
        FeaturePipeline.from_state(other, state)
    # ... and the reverse: the schema has a categorical column the pipeline never saw
    more = parse_schema(NAMES + ",rig", TYPES + ",string")
    with pytest.raises(ValueError, match="'rig'"):
        FeaturePipeline.from_state(more, state)
    with pytest.raises(ValueError, match=rf"{pipe.n_features}.*99|99.*{pipe.n_features}"):
        FeaturePipeline.from_state(schema, state, n_features=99)


# ------------------------------------------------------------------ 2. codes()
@pytest.mark.parametrize("handle_invalid", ["keep", "skip"])
def test_codes_equals_transform(handle_invalid):
    ix = StringIndexer("c", handle_invalid=handle_invalid).fit(["a", "b", "b", 3, 3, 3, 2.5, "2.5", "zz", 7])
    cases = [
        ["b", "a", "b", "b", "nope", 3, "3", 2.5, 7.0, 7, "zz", None, "", "a"],
        np.asarray(["a", "q", "b", "a"], dtype=object),
        np.asarray(["a", "q", "b", "a"]),
        np.asarray([3, 7, 8, 3, 3], np.int64),
        np.asarray([2.5, 3.0, 7.0, 2.5], np.float32),
        [],
    ]
    for vals in cases:
        got, want = ix.codes(vals), ix.transform(vals)
        assert got.dtype == np.int32 and np.array_equal(got, want), (vals, got, want)
    assert ix.codes(["nope"])[0] == len(ix.labels)  # unseen -> the extra index
    strict = StringIndexer("c", labels=["a"], handle_invalid="error")
    with pytest.raises(ValueError, match="unseen"):
        strict.codes(["a", "x"])


# ------------------------------------------------------------------ 3. raw columns + kernel semantics
def emulate_assembly(codes, cont, off, size, mean, std, F, ld):
    """csrc/features.hip in numpy: one-hot blocks, then (x - mean) / std in fp32, zero padding."""
    n = codes.shape[1] if len(codes) else cont.shape[1]
    out = np.zeros((n, ld), np.float32)
    for c in range(len(codes)):
        ok = codes[c] < size[c]
        out[np.nonzero(ok)[0], off[c] + codes[c][ok]] = 1.0
    Fc = F - len(cont)
    for q in range(len(cont)):
        out[:, Fc + q] = (cont[q] - mean[q]) / std[q]
    return out


@pytest.mark.parametrize("standardize", [True, False])
def test_raw_columns_pin_the_block_spec(standardize):
    schema = _schema()
    table = _synth(6, 100)
    pipe = FeaturePipeline(schema, "flow", standardize=standardize).fit(take(table, np.arange(250)))
    codes, cont = pipe.raw_columns(table)
    off, size = pipe.block_spec()
    mean, std = pipe.scale()
    assert codes.dtype == np.int32 and codes.shape == (2, 600)
    assert cont.dtype == np.float32 and cont.shape == (7, 600)  # 't' (int) is cast on the host
    assert off.dtype == np.int32 and size.dtype == np.int32 and mean.dtype == np.float32 and std.dtype == np.float32
    # 3 training wells -> 3 labels + unknown - dropped last = 3 columns; 3 fields likewise
    assert size.tolist() == [3, 3] and off.tolist() == [0, 3]
    assert codes[0].max() == 3  # wells unseen in training carry the unknown index
    F = pipe.n_features
    X = pipe.transform(table)[0]
    assert np.array_equal(emulate_assembly(codes, cont, off, size, mean, std, F, F), X)
    padded = emulate_assembly(codes, cont, off, size, mean, std, F, 24)
    assert np.array_equal(padded[:, :F], X) and not padded[:, F:].any()
    if not standardize:
        assert not mean.any() and (std == 1).all()


# ------------------------------------------------------------------ helpers for the jobs
def _csv(tmp_path, table, name="data.csv", order=None):
    t = table if order is None else take(table, order)
    t = {k: (np.asarray(v, dtype=object) if np.asarray(v).dtype.kind in "OU" else np.asarray(v)) for k, v in t.items()}
    path = str(tmp_path / name)
    write_csv(t, path, columns=NAMES.split(","))
    return path, load_table(path, _schema())  # what the job will parse


def _oracle(mdl_path, schema):
    from wellflow.config import MODEL_DEFAULTS, RunConfig
    from wellflow.predict import model_shapes

    name, layers, extra = load_mdl(mdl_path)
    shp = model_shapes(name, layers)
    cfg = RunConfig(model=name, **MODEL_DEFAULTS[name])
    for k, v in shp.items():
        if k != "n_features":
            setattr(cfg, k, v)
    ref = registry.build_reference(name, cfg, shp["n_features"], shp.get("cnn_outputs", 1))
    registry.load_keras_layers(name, ref, layers)
    ref.eval()
    return ref, FeaturePipeline.from_state(schema, extra["features"]), extra


# ------------------------------------------------------------------ 4. MLP job
def test_mlp_job_scores_a_csv(tmp_path):
    from wellflow.predict import run_predict
    from wellflow.train.job import run_job

    sp = str(tmp_path) + "/"
    run_job("mlp", [NAMES, TYPES, "flow", sp, "--device", "cpu", "--precision", "fp32", "--max-steps", "30",
                    "--synth-wells", "4", "--synth-steps", "200", "--verbose", "0"], **QUIET)
    path, table = _csv(tmp_path, _synth(4, 200))
    lines = []
    res = run_predict("mlp", [NAMES, TYPES, "flow", sp, path, "--device", "cpu", "--precision", "fp32"],
                      log=lambda s: lines.append(str(s)))
    assert res["out"] == sp + "predictions/mlp.csv" and not os.path.exists(res["out"] + ".tmp")
    rows = _read_out(res["out"])
    assert len(rows) == 800 and all(len(r) == 11 for r in rows)
    _assert_echo(rows, table, NAMES.split(","))
    ref, pipe, extra = _oracle(sp + "models/mlp.mdl", _schema())
    assert extra["job"]["mlp_hidden"] == [256, 256] and extra["job"]["seq_len"] == 64
    with torch.no_grad():
        want = pipe.inverse_target(ref(torch.from_numpy(pipe.transform(table)[0])).numpy())
    got = _pred_col(rows)
    assert np.allclose(got, want, rtol=1e-5, atol=0), np.abs(got / want - 1).max()
    assert np.allclose(res["predictions"], want, rtol=1e-5, atol=0)
    mse = float(np.mean((res["predictions"].astype(np.float64) - table["flow"].astype(np.float64)) ** 2))
    assert res["mse"] == mse and res["scored"] == 800 and res["unscored"] == 0
    assert "Rows scored: 800" in lines and "Rows without prediction: 0" in lines
    assert "Scoring MSE: %f" % mse in lines

    # the data need not hold the target: same predictions, no MSE line
    names9, types9 = NAMES.rsplit(",", 1)[0], TYPES.rsplit(",", 1)[0]
    p9 = str(tmp_path / "nine.csv")
    write_csv({k: (np.asarray(v, dtype=object) if np.asarray(v).dtype == object else v) for k, v in table.items()},
              p9, columns=names9.split(","))
    lines9 = []
    res9 = run_predict("mlp", [names9, types9, "flow", sp, p9, "--device", "cpu", "--precision", "fp32", "--out",
                               str(tmp_path / "o9.csv")], log=lambda s: lines9.append(str(s)))
    assert np.array_equal(res9["predictions"], res["predictions"]) and res9["mse"] is None
    assert not any(l.startswith("Scoring MSE") for l in lines9)
    assert len(_read_out(str(tmp_path / "o9.csv"))[0]) == 10


def test_submit_dispatches_predict(tmp_path, capsys):
    from wellflow import submit
    from wellflow.train.job import run_job

    sp = str(tmp_path) + "/"
    run_job("gilbert", [NAMES, TYPES, "flow", sp, "--synth-wells", "2", "--synth-steps", "50"], **QUIET)
    path, table = _csv(tmp_path, _synth(2, 50))
    assert submit.main(["predict", "gilbert", NAMES, TYPES, "flow", sp, path]) == 0
    assert "Rows scored: 100" in capsys.readouterr().out
    assert len(_read_out(sp + "predictions/gilbert.csv")) == 100


# ------------------------------------------------------------------ 5. LSTM
def test_lstm_scores_interleaved_series(tmp_path):
    from wellflow.predict import run_predict
    from wellflow.train.job import run_job

    sp = str(tmp_path) + "/"
    T = 8
    run_job("lstm", [NAMES, TYPES, "flow", sp, "--device", "cpu", "--precision", "fp32", "--seq-len", str(T),
                     "--hidden", "32", "--synth-wells", "3", "--synth-steps", "40", "--epochs", "2", "--verbose", "0"],
            **QUIET)
    base = _synth(3, 40)
    inter = np.arange(120).reshape(3, 40).T.ravel()  # t0 of every well, t1 of every well, ...
    path, table = _csv(tmp_path, base, order=inter)
    assert list(table["well"][:4]) == ["W000", "W001", "W002", "W000"]
    # the saved job settings win over argv (no --seq-len / --hidden here)
    res = run_predict("lstm", [NAMES, TYPES, "flow", sp, path, "--device", "cpu", "--precision", "fp32"], **QUIET)
    ref, pipe, extra = _oracle(sp + "models/lstm.mdl", _schema())
    assert extra["job"]["seq_len"] == T and extra["job"]["hidden"] == 32 and extra["job"]["group_col"] == "well"

    def expected(tab):
        X = torch.from_numpy(pipe.transform(tab)[0])
        want = np.full(len(X), np.nan, np.float32)
        wells = np.asarray(tab["well"]).astype(str)
        for w in np.unique(wells):
            pos = np.flatnonzero(wells == w)  # file order = time order inside the well
            for i in range(T - 1, len(pos)):
                with torch.no_grad():
                    p = ref(X[pos[i - T + 1 : i + 1]][None])
                want[pos[i]] = pipe.inverse_target(p.numpy())[0]
        return want

    want = expected(table)
    got = res["predictions"]
    nan = np.isnan(got)
    assert nan.sum() == 3 * (T - 1) and np.array_equal(np.flatnonzero(nan), np.arange(21))  # first 7 rows per well
    assert np.array_equal(nan, np.isnan(want))
    assert np.allclose(got[~nan], want[~nan], rtol=1e-5, atol=1e-5 * np.abs(want[~nan]).max())
    assert res["scored"] == 99 and res["unscored"] == 21
    rows = _read_out(res["out"])
    assert len(rows) == 120 and sum(r[-1] == "" for r in rows) == 21
    assert np.allclose(_pred_col(rows)[~nan], got[~nan], rtol=1e-6)

    # a well shorter than the window, mixed into the file: 5 more NaN, nothing else moves
    short = take(_synth(4, 40), np.arange(120, 125))
    short["well"] = np.asarray(["W9"] * 5, dtype=object)
    both = {k: np.concatenate([np.asarray(table[k], dtype=object if np.asarray(table[k]).dtype == object else None),
                               np.asarray(short[k])]) for k in table}
    mix = np.concatenate([np.arange(50), [120, 121], np.arange(50, 100), [122, 123, 124], np.arange(100, 120)])
    path2, table2 = _csv(tmp_path, both, name="mixed.csv", order=mix)
    res2 = run_predict("lstm", [NAMES, TYPES, "flow", sp, path2, "--device", "cpu", "--precision", "fp32", "--out",
                                str(tmp_path / "mixed_out.csv")], **QUIET)
    got2 = res2["predictions"]
    is_short = np.asarray(table2["well"]).astype(str) == "W9"
    assert is_short.sum() == 5 and np.isnan(got2[is_short]).all()
    assert np.array_equal(got2[~is_short], got, equal_nan=True)
    assert res2["unscored"] == 26


# ------------------------------------------------------------------ 6. CNN
def test_cnn_forecasts_every_window(tmp_path):
    from wellflow.models.cnn import CNN1DRegressor
    from wellflow.predict import Predictor, run_predict

    schema = _schema()
    L, O = 48, 12
    path, table = _csv(tmp_path, _synth(2, 100))
    pipe = FeaturePipeline(schema, "flow", standardize_target=True).fit(table)
    ref = CNN1DRegressor(L, 1, 100, 13, O).init_keras(5)
    sp = str(tmp_path) + "/"
    save_mdl(sp + "models/cnn.mdl", "cnn", registry.keras_layers("cnn", ref), {"features": pipe.state()})
    pred = Predictor.load(sp + "models/cnn.mdl", schema, device="cpu", precision="fp32")
    assert (pred.cfg.cnn_input_len, pred.cfg.cnn_outputs, pred.cfg.cnn_filters, pred.cfg.cnn_kernel) == (L, O, 100, 13)
    end_rows, fc = pred.predict_table(table)
    assert fc.shape == (2 * 53, O) and end_rows.shape == (106,)
    # windows end at rows 47 .. 99 of each well; the last 12 per well forecast past the data
    assert np.array_equal(end_rows, np.concatenate([np.arange(47, 100), np.arange(147, 200)]))
    y = pipe.target_values(table)
    ref.eval()
    with torch.no_grad():
        X = torch.from_numpy(np.stack([y[e - L + 1 : e + 1] for e in end_rows]))[:, :, None]
        want = pipe.inverse_target(ref(X).numpy())
    assert np.allclose(fc, want, rtol=1e-5, atol=1e-5 * np.abs(want).max())

    res = run_predict("cnn", [NAMES, TYPES, "flow", sp, path, "--device", "cpu", "--precision", "fp32"], **QUIET)
    rows = _read_out(res["out"])
    assert len(rows) == 200 and all(len(r) == 10 + O for r in rows)
    filled = np.asarray([r[10] != "" for r in rows])
    assert np.array_equal(np.flatnonzero(filled), end_rows) and res["scored"] == 106
    assert np.allclose(_pred_col(rows, 10 + O - 1)[filled], fc[:, O - 1], rtol=1e-6)
    # MSE over the 2 x 41 x 12 forecast cells whose horizon rows exist
    d = []
    for e, f in zip(end_rows, fc):
        hi = 100 if e < 100 else 200
        k = min(O, hi - 1 - e)
        d.append(f[:k].astype(np.float64) - table["flow"][e + 1 : e + 1 + k].astype(np.float64))
    d = np.concatenate(d)
    assert np.isclose(res["mse"], np.mean(d * d), rtol=1e-12)


# ------------------------------------------------------------------ 7. Gilbert
def test_gilbert_scores_with_the_saved_correlation(tmp_path):
    from wellflow.models.gilbert import GilbertModel
    from wellflow.predict import Predictor

    table = _synth(2, 30)
    p = str(tmp_path / "models" / "gilbert.mdl")
    save_mdl(p, "gilbert", [("Gilbert", [torch.tensor([17.4, 0.5, 2.0])])], {"correlation": "ros", "glr_unit": "scf"})
    got = Predictor.load(p, _schema(), device="cpu").predict_table(table)
    want = GilbertModel(correlation="ros").predict({k: np.asarray(table[k], np.float64) for k in ("whp", "choke", "glr")})
    assert got.shape == (60,) and np.array_equal(got, want)
    assert not np.array_equal(got, GilbertModel().predict({k: np.asarray(table[k], np.float64)
                                                           for k in ("whp", "choke", "glr")}))


# ------------------------------------------------------------------ 8. errors
def _mlp_layers(F, hidden=(16, 8), seed=0):
    from wellflow.models.mlp import MLPRegressor

    torch.manual_seed(seed)
    ref = MLPRegressor(F, hidden)
    return ref, registry.keras_layers("mlp", ref)


def test_predict_errors_name_the_cause(tmp_path):
    from wellflow.predict import Predictor

    schema = _schema()
    table = _synth(3, 20)
    pipe = FeaturePipeline(schema, "flow", standardize_target=True).fit(table)
    F = pipe.n_features
    missing = str(tmp_path / "models" / "mlp.mdl")
    with pytest.raises(FileNotFoundError, match="mlp.mdl"):
        Predictor.load(missing, schema, device="cpu")
    ref, layers = _mlp_layers(F)
    bare = str(tmp_path / "bare.mdl")
    save_mdl(bare, "mlp", layers, {"epoch": 1})
    with pytest.raises(ValueError, match="features"):
        Predictor.load(bare, schema, device="cpu")
    _, narrow = _mlp_layers(F - 3)
    wrong = str(tmp_path / "wrong.mdl")
    save_mdl(wrong, "mlp", narrow, {"features": pipe.state()})
    with pytest.raises(ValueError, match=rf"{F}\b.*\b{F - 3}\b|{F - 3}\b.*\b{F}\b"):
        Predictor.load(wrong, schema, device="cpu")


def test_round1_safetensors_mdl_still_scores(tmp_path):
    from safetensors.torch import save_file
    from wellflow.predict import Predictor

    schema = _schema()
    table = _synth(3, 20)
    pipe = FeaturePipeline(schema, "flow", standardize_target=True).fit(table)
    ref, layers = _mlp_layers(pipe.n_features)
    tensors, meta = {}, {"model": "mlp", "nb_layers": str(len(layers)), "extra": json.dumps({"features": pipe.state()})}
    for k, (cls, params) in enumerate(layers):
        meta[f"layer_{k}/nb_params"], meta[f"layer_{k}/class"] = str(len(params)), cls
        for n, t in enumerate(params):
            tensors[f"layer_{k}/param_{n}"] = t.detach().contiguous().clone()
    p = str(tmp_path / "old.mdl")
    save_file(tensors, p, metadata=meta)
    pred = Predictor.load(p, schema, device="cpu", precision="fp32")
    assert pred.cfg.mlp_hidden == (16, 8)
    got = pred.predict_table(table)
    with torch.no_grad():
        want = pipe.inverse_target(ref(torch.from_numpy(pipe.transform(table)[0])).numpy())
    assert got.shape == (60,) and np.allclose(got, want, rtol=1e-5, atol=1e-5 * np.abs(want).max())
