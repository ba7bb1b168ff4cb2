"""Shapley attribution on the CPU (fp32 oracle engines, host float64): the rule against an independent
numpy float64 replay bit for bit, local accuracy, the exact zeros, the exact Shapley value of
Gilbert's equation at full enumeration, seeding, the per-family semantics and the job's CSV / stdout
contract (wellflow/explain.py)."""
import csv
import itertools
import math
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
EPS = 2.0 ** -52


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


def _draws(n, R, K, seed):
    rng = np.random.default_rng(seed)
    orders = np.stack([rng.permutation(K) for _ in range(R)])
    perms = np.stack([rng.permutation(n) for _ in range(R)])
    return orders, perms


def replay(score, names, picked, orders, perms, y_scale, y_shift):
    """The rule of the issue, written out on its own: ``score(columns, perm)`` -> fp32 outputs of
    the table with those columns read through perm. Returns phi, std [K][M], base, base_std [M]."""
    R, K = orders.shape
    p_full = np.asarray(score([], None))
    M = len(p_full)
    acc, sq = np.zeros((K + 1, M)), np.zeros((K + 1, M))
    for r in range(R):
        left = [picked[k] for k in orders[r]]
        p_prev = np.asarray(score(left, perms[r])).astype(np.float64)
        v = p_prev * y_scale + y_shift
        acc[K] += v
        sq[K] += v * v
        for j in range(K):
            left = left[1:]
            p_cur = (p_full if j == K - 1 else np.asarray(score(left, perms[r]))).astype(np.float64)
            d = (p_cur - p_prev) * y_scale
            acc[orders[r, j]] += d
            sq[orders[r, j]] += d * d
            p_prev = p_cur
    mean = acc / R
    std = np.sqrt(np.maximum(0.0, sq / R - mean * mean))
    return mean[:K], std[:K], mean[K], std[K], p_full.astype(np.float64) * y_scale + y_shift


def _local_accuracy(res):
    K = len(res["columns"])
    gap = np.abs(res["base"] + res["phi"].sum(axis=0) - res["prediction"])
    scale = np.maximum(np.maximum(np.abs(res["base"]), np.abs(res["prediction"])), np.abs(res["phi"]).sum(axis=0))
    bound = 4 * (K + 1) * EPS * scale
    print("local accuracy: max gap / bound", float((gap / np.maximum(bound, 1e-300)).max()))
    assert (gap <= bound).all(), float((gap / bound).max())


@pytest.fixture(scope="module")
def mlp(tmp_path_factory):
    """MLPRegressor(18, (256, 256)) on the synthetic table (8 wells x 125 steps, F = 18); the first
    layer ignores the 'field' one-hot block (columns 8 .. 10). One injected run is shared."""
    from wellflow.explain import ShapleyAttribution
    from wellflow.models.mlp import MLPRegressor
    from wellflow.predict import Predictor

    d = tmp_path_factory.mktemp("explain_mlp")
    schema = _schema()
    path, table = _csv_file(d, _synth(8, 125))
    pipe = FeaturePipeline(schema, "flow", standardize_target=True).fit(table)
    assert pipe.n_features == 18 and [ix.column for ix in pipe.indexers] == ["well", "field"]
    torch.manual_seed(0)
    ref = MLPRegressor(18, (256, 256))
    with torch.no_grad():
        ref.linears()[0].weight[:, 8:11] = 0.0
    sp = str(d) + "/"
    save_mdl(sp + "models/mlp.mdl", "mlp", registry.keras_layers("mlp", ref), {"features": pipe.state()})
    ref.eval()
    pred = Predictor.load(sp + "models/mlp.mdl", schema, device="cpu", precision="fp32")
    orders, perms = _draws(1000, 2, 9, 5)
    res = ShapleyAttribution(pred, repeats=2).run(table, orders=orders, perms=perms)
    return dict(sp=sp, path=path, table=table, pipe=pipe, ref=ref, schema=schema, pred=pred, orders=orders, perms=perms,
                res=res)


# ------------------------------------------------------------------ 1. the rule
def test_mlp_rule_equals_numpy_replay_bit_for_bit(mlp):
    table, pipe, ref, res = mlp["table"], mlp["pipe"], mlp["ref"], mlp["res"]
    assert res["columns"] == INPUTS and not res["native"] and res["scored"] == 1000
    assert res["rows"].tolist() == list(range(1000))

    def score(cols, perm):
        t2 = dict(table)
        for c in cols:
            t2[c] = np.asarray(table[c])[perm]
        with torch.no_grad():
            return ref(torch.from_numpy(pipe.features(t2))).reshape(-1).numpy()

    phi, std, base, base_std, prediction = replay(score, INPUTS, INPUTS, mlp["orders"], mlp["perms"],
                                                  float(pipe.y_std), float(pipe.y_mean))
    for name, want in (("phi", phi), ("std", std), ("base", base), ("base_std", base_std), ("prediction", prediction)):
        assert res[name].dtype == np.float64 and res[name].shape == want.shape
        assert np.array_equal(res[name].view(np.int64), want.view(np.int64)), name
    assert np.array_equal(res["mean_abs"], np.abs(phi).mean(axis=1)) and (res["mean_abs"][[0, 3, 4]] > 0).all()
    y = pipe.target_values(table, raw=True).astype(np.float64)
    assert np.isclose(res["mse"], np.mean((prediction - y) ** 2), rtol=1e-12)


# ------------------------------------------------------------------ 2. local accuracy
def test_local_accuracy(mlp):
    _local_accuracy(mlp["res"])


# ------------------------------------------------------------------ 3. exact zeros
def test_unread_column_and_identity_perm_give_exact_zeros(mlp):
    from wellflow.explain import ShapleyAttribution

    res = mlp["res"]
    k = res["columns"].index("field")
    assert (res["phi"][k] == 0.0).all() and (res["std"][k] == 0.0).all()
    ident = ShapleyAttribution(mlp["pred"], repeats=2).run(mlp["table"], orders=mlp["orders"],
                                                           perms=np.stack([np.arange(1000)] * 2))
    assert (ident["phi"] == 0.0).all() and (ident["std"] == 0.0).all()
    assert np.array_equal(ident["base"], ident["prediction"]) and np.array_equal(ident["prediction"], res["prediction"])


# ------------------------------------------------------------------ 4. exact Shapley on Gilbert
def test_gilbert_full_enumeration_is_the_exact_shapley_value(tmp_path):
    from wellflow.explain import ShapleyAttribution
    from wellflow.models.gilbert import GilbertModel
    from wellflow.predict import Predictor

    table = dict(_synth(4, 125))
    n = 500
    p = str(tmp_path / "models" / "gilbert.mdl")
    save_mdl(p, "gilbert", [("Gilbert", [torch.tensor([17.4, 0.5, 2.0])])], {"correlation": "ros", "glr_unit": "scf"})
    orders = np.asarray(list(itertools.permutations(range(3))))
    perm = np.random.default_rng(8).permutation(n)
    job = ShapleyAttribution(Predictor.load(p, _schema(), device="cpu"), repeats=6)
    res = job.run(table, orders=orders, perms=np.stack([perm] * 6))  # no target column is needed
    assert res["columns"] == ["whp", "choke", "glr"] and res["scored"] == n and not res["native"] and res["mse"] is None
    # the subset-weight formula, by brute force over the 8 coalitions
    model = GilbertModel(correlation="ros")
    own = {k: np.asarray(table[k], np.float64) for k in ("whp", "choke", "glr")}
    names = ["whp", "choke", "glr"]

    def v(S):
        return model.predict({c: own[c] if i in S else own[c][perm] for i, c in enumerate(names)})

    vs = {S: v(S) for m in range(4) for S in itertools.combinations(range(3), m)}
    vmax = np.max(np.abs(np.stack(list(vs.values()))), axis=0)
    for i in range(3):
        want = np.zeros(n)
        for S in vs:
            if i not in S:
                w = math.factorial(len(S)) * math.factorial(3 - len(S) - 1) / math.factorial(3)
                want += w * (vs[tuple(sorted(S + (i,)))] - vs[S])
        err = np.abs(res["phi"][i] - want) / (EPS * vmax)
        print(f"gilbert {names[i]}: max |phi - shapley| = {err.max():.3g} x 2^-52 x max|v(S)|")
        assert (err <= 16).all(), err.max()
    assert np.allclose(res["base"], vs[()], rtol=8 * EPS, atol=0)  # six equal terms added, then / 6
    assert np.array_equal(res["prediction"], vs[(0, 1, 2)]) and (np.abs(res["phi"]).max(axis=1) > 0).all()
    _local_accuracy(res)
    with pytest.raises(ValueError, match="whp, choke, glr"):
        job.run(table, columns=["temp"])


# ------------------------------------------------------------------ 5. seeding
def test_seed_decides_the_draws(mlp):
    from wellflow.explain import ShapleyAttribution

    table, cols = take(mlp["table"], np.arange(200)), ["whp", "choke", "well"]
    a, b, c = (ShapleyAttribution(mlp["pred"], repeats=2, seed=s).run(table, columns=cols) for s in (5, 5, 6))
    assert np.array_equal(a["phi"], b["phi"]) and np.array_equal(a["base"], b["base"])
    assert np.array_equal(a["orders"], b["orders"])
    assert np.array_equal(a["prediction"], c["prediction"]) and not np.array_equal(a["phi"], c["phi"])
    assert not np.array_equal(a["base"], c["base"])


# ------------------------------------------------------------------ 6. --columns
def test_unpicked_columns_never_move(mlp):
    from wellflow.explain import ShapleyAttribution

    table, pipe, ref = mlp["table"], mlp["pipe"], mlp["ref"]
    orders, perms = _draws(1000, 2, 3, 12)
    # named out of source order: kept in source order, which is what `orders` indexes
    res = ShapleyAttribution(mlp["pred"], repeats=2).run(table, columns=["choke", "well", "whp"], orders=orders, perms=perms)
    assert res["columns"] == ["well", "whp", "choke"] and res["phi"].shape == (3, 1000)
    seen = []

    def score(cols, perm):
        seen.append(tuple(cols))
        t2 = dict(table)
        for c in cols:
            t2[c] = np.asarray(table[c])[perm]
        with torch.no_grad():
            return ref(torch.from_numpy(pipe.features(t2))).reshape(-1).numpy()

    phi, _, base, _, prediction = replay(score, INPUTS, ["well", "whp", "choke"], orders, perms, float(pipe.y_std),
                                         float(pipe.y_mean))
    assert set(c for s in seen for c in s) == {"well", "whp", "choke"}  # the replay moved nothing else either
    assert np.array_equal(res["phi"], phi) and np.array_equal(res["base"], base)
    assert np.array_equal(res["prediction"], mlp["res"]["prediction"])
    _local_accuracy(res)


# ------------------------------------------------------------------ 7. LSTM
def test_lstm_cyclic_shift_rows_and_empty_cells(tmp_path):
    from wellflow.explain import ShapleyAttribution, run_explain
    from wellflow.models.lstm import LSTMRegressor
    from wellflow.predict import Predictor

    T, H = 8, 16
    schema = _schema()
    base = _synth(3, 40)
    inter = np.arange(120).reshape(3, 40).T.ravel()  # t0 of every well, t1 of every well, ...
    path, table = _csv_file(tmp_path, base, order=inter)
    pipe = FeaturePipeline(schema, "flow").fit(table)  # target left raw: predictions are network outputs
    torch.manual_seed(2)
    ref = LSTMRegressor(pipe.n_features, H)
    sp = str(tmp_path) + "/"
    save_mdl(sp + "models/lstm.mdl", "lstm", registry.keras_layers("lstm", ref),
             {"features": pipe.state(), "job": {"seq_len": T, "group_col": "well", "hidden": H}})
    pred = Predictor.load(sp + "models/lstm.mdl", schema, device="cpu", precision="fp32")
    n, R, cols = 120, 2, ["well", "whp", "choke"]
    res = ShapleyAttribution(pred, repeats=R, seed=4).run(table, columns=cols)
    assert res["scored"] == 3 * (40 - T + 1) == 99 and res["n"] == 120
    # the default draws: the orders, then the shifts, from the host generator
    rng = np.random.default_rng(4)
    orders = np.stack([rng.permutation(3) for _ in range(R)])
    shifts = rng.integers(1, n, size=R)
    assert np.array_equal(res["orders"], orders) and ((1 <= shifts) & (shifts <= n - 1)).all()
    perms = np.stack([(np.arange(n) + s) % n for s in shifts])
    # the map acts on the series-sorted table; a window's prediction belongs to its last row
    ids = np.unique(np.asarray(table["well"]).astype(str), return_inverse=True)[1]
    order = np.argsort(ids, kind="stable")
    stable = take(table, order)
    starts = np.asarray(window_starts(n, T, ids[order]))
    assert np.array_equal(res["rows"], order[starts + T - 1])
    ref.eval()

    def score(picked, perm):
        t2 = dict(stable)
        for c in picked:
            t2[c] = np.asarray(stable[c])[perm]
        X = pipe.features(t2)
        with torch.no_grad():
            return ref(torch.from_numpy(X[starts[:, None] + np.arange(T)[None, :]])).reshape(-1).numpy()

    phi, _, base_, _, prediction = replay(score, INPUTS, cols, orders, perms, 1.0, 0.0)
    assert np.allclose(res["phi"], phi, rtol=1e-5, atol=1e-6) and np.allclose(res["base"], base_, rtol=1e-5, atol=1e-6)
    assert np.abs(res["phi"]).max() > 0
    _local_accuracy(res)
    out = pred.predict_table(table)
    assert np.allclose(out[res["rows"]], res["prediction"], rtol=1e-6) and np.isnan(out).sum() == 21
    # the job: the unscored rows (the first T - 1 of every series) get empty cells
    lines = []
    job = run_explain("lstm", [NAMES, TYPES, "flow", sp, path, *CPU, "--repeats", "2", "--columns", "whp,choke"],
                      log=lambda s: lines.append(str(s)))
    assert lines[0] == "Rows scored: 99" and lines[1] == "Rows without prediction: 21"
    head, rows = _read(job["out"])
    assert head == NAMES.split(",") + ["prediction", "base", "phi_whp", "phi_choke"] and len(rows) == 120
    empty = [i for i, r in enumerate(rows) if r[10] == ""]
    assert sorted(empty) == sorted(set(range(120)) - set(res["rows"].tolist())) and len(empty) == 21
    assert all(r[10:] == [""] * 4 for i, r in enumerate(rows) if i in empty)
    assert all("" not in r[10:] for i, r in enumerate(rows) if i not in empty)
    with pytest.raises(ValueError, match="shorter than the window"):
        ShapleyAttribution(pred).run(take(table, np.arange(15)))


# ------------------------------------------------------------------ 8. refusals
def test_refusals_name_the_cause(mlp, tmp_path):
    from wellflow.explain import ShapleyAttribution, run_explain
    from wellflow.models.cnn import CNN1DRegressor

    table, pred = mlp["table"], mlp["pred"]
    job = ShapleyAttribution(pred, repeats=2)
    good_o, good_p = _draws(1000, 2, 9, 1)
    with pytest.raises(ValueError, match=r"orders must be \[2\]\[9\]"):
        job.run(table, orders=good_o[:1], perms=good_p)
    with pytest.raises(ValueError, match=r"orders must be \[2\]\[3\]"):
        job.run(table, columns=["whp", "choke", "glr"], orders=good_o, perms=good_p)
    bad = good_o.copy()
    bad[1, 0] = bad[1, 1]
    with pytest.raises(ValueError, match=r"orders\[1\] .* is not a permutation of 0 \.\. 8"):
        job.run(table, orders=bad, perms=good_p)
    with pytest.raises(TypeError, match="orders must be integers"):
        job.run(table, orders=good_o.astype(np.float64), perms=good_p)
    with pytest.raises(ValueError, match=r"perms must be \[2\]\[1000\]"):
        job.run(table, orders=good_o, perms=good_p[:, :999])
    with pytest.raises(ValueError, match=r"perms\(0\) gave \(999,\), not \[1000\]"):
        job.run(table, orders=good_o, perms=lambda r: good_p[r, :999])
    with pytest.raises(TypeError, match="perms: a tensor"):
        job.run(table, orders=good_o, perms=[1, 2])
    with pytest.raises(ValueError, match="unknown column 'nope'"):
        job.run(table, columns=["nope"])
    with pytest.raises(ValueError, match="unknown column 'flow'"):  # the target is no input
        job.run(table, columns=["flow"])
    with pytest.raises(ValueError, match="column 'whp' listed twice"):
        job.run(table, columns=["whp", "choke", "whp"])
    with pytest.raises(ValueError, match="lacks the input column 'glr'"):
        job.run({k: v for k, v in table.items() if k != "glr"})
    with pytest.raises(ValueError, match="repeats must be >= 1"):
        ShapleyAttribution(pred, repeats=0)
    # the target column is not required
    no_target = ShapleyAttribution(pred, repeats=1).run({k: v[:50] for k, v in table.items() if k != "flow"},
                                                       columns=["whp"])
    assert no_target["mse"] is None and no_target["phi"].shape == (1, 50)
    # cnn: refused with the importance job's reason, nothing written
    path, t2 = _csv_file(tmp_path, _synth(2, 100))
    pipe = FeaturePipeline(_schema(), "flow", standardize_target=True).fit(t2)
    ref = CNN1DRegressor(48, 1, 100, 13, 12).init_keras(5)
    sp = str(tmp_path) + "/"
    save_mdl(sp + "models/cnn.mdl", "cnn", registry.keras_layers("cnn", ref), {"features": pipe.state()})
    with pytest.raises(ValueError, match="target's own history.*no input column"):
        run_explain("cnn", [NAMES, TYPES, "flow", sp, path, *CPU], **QUIET)
    assert not os.path.exists(sp + "explain/cnn.csv")


# ------------------------------------------------------------------ 9. the job
def test_job_csv_layout_stdout_and_rank(mlp, tmp_path, monkeypatch):
    from wellflow.explain import run_explain

    sp, path = mlp["sp"], mlp["path"]
    args = [NAMES, TYPES, "flow", sp, path, *CPU, "--repeats", "2", "--seed", "7"]
    lines = []
    a = run_explain("mlp", args, log=lambda s: lines.append(str(s)))
    assert a["out"] == sp + "explain/mlp.csv" and not os.path.exists(a["out"] + ".tmp")
    head, rows = _read(a["out"])
    assert head == NAMES.split(",") + ["prediction", "base"] + ["phi_" + c for c in INPUTS] and len(rows) == 1000
    vals = np.asarray([[float(v) for v in r[10:]] for r in rows])
    assert np.array_equal(vals[:, 0], a["prediction"]) and np.array_equal(vals[:, 1], a["base"])  # repr round-trips
    assert np.array_equal(vals[:, 2:].T, a["phi"])
    assert [r[0] for r in rows] == [str(v) for v in mlp["table"]["well"]]  # the table is echoed
    assert np.allclose([float(r[3]) for r in rows], mlp["table"]["whp"], rtol=1e-6)
    gap = np.abs(vals[:, 1] + vals[:, 2:].sum(axis=1) - vals[:, 0])
    assert (gap <= 1e-9 * np.abs(vals[:, 0])).all()
    assert lines[0] == "Rows scored: 1000" and lines[1] == "Rows without prediction: 0"
    assert lines[2] == "Mean prediction: %f" % a["prediction"].mean() and lines[3] == "Scoring MSE: %f" % a["mse"]
    shown = [l.split(":")[0] for l in lines[4:]]
    assert len(lines) == 13 and sorted(shown) == sorted(INPUTS) and shown[-1] == "field"
    ma = dict(zip(a["columns"], a["mean_abs"]))
    assert [ma[c] for c in shown] == sorted(ma.values(), reverse=True)
    # the same seed writes the same file; --std adds the spread columns; --columns picks
    with open(a["out"], "rb") as f:
        first = f.read()
    b = run_explain("mlp", args + ["--out", str(tmp_path / "again.csv")], **QUIET)
    with open(tmp_path / "again.csv", "rb") as f:
        assert f.read() == first and b["out"] == str(tmp_path / "again.csv")
    s = run_explain("mlp", args + ["--std", "--columns", "choke,well", "--out", str(tmp_path / "std.csv")], **QUIET)
    head, rows = _read(str(tmp_path / "std.csv"))
    assert head[10:] == ["prediction", "base", "phi_well", "phi_choke", "std_well", "std_choke"]
    assert np.array_equal(np.asarray([float(r[15]) for r in rows]), s["std"][1])
    # under torchrun, rank 0 alone works and writes
    monkeypatch.setenv("RANK", "1")
    skipped = run_explain("mlp", args + ["--out", str(tmp_path / "rank1.csv")], **QUIET)
    assert skipped["skipped"] and not os.path.exists(tmp_path / "rank1.csv")


def test_submit_dispatches_explain(tmp_path, capsys):
    from wellflow import submit
    from wellflow.train.job import run_job

    sp = str(tmp_path) + "/"
    run_job("gilbert", [NAMES, TYPES, "flow", sp, "--synth-wells", "2", "--synth-steps", "50"], **QUIET)
    path, table = _csv_file(tmp_path, _synth(2, 50))
    assert submit.main(["explain", "gilbert", NAMES, TYPES, "flow", sp, path, "--repeats", "2"]) == 0
    out = capsys.readouterr().out
    assert "Rows scored: 100" in out and "Mean prediction: " in out and "Scoring MSE: " in out
    head, rows = _read(sp + "explain/gilbert.csv")
    assert head[10:] == ["prediction", "base", "phi_whp", "phi_choke", "phi_glr"] and len(rows) == 100
