"""Set points on the CPU (fp32 oracle engines, Gilbert in float64): the numpy rule against a
per-element loop bit for bit, Gilbert's closed form, the reality of a bracket (re-scoring at lo and
hi gives f_lo and f_hi), the per-family semantics and the job's CSV / stdout contract
(wellflow/setpoint.py)."""
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
TAIL = ["prediction", "wanted", "setpoint", "status", "lo", "hi", "miss"]
NAN = float("nan")


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


def same_bits(a, b):
    """Equal bit for bit where neither is NaN, and NaN at the same positions."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    na, nb = np.isnan(a), np.isnan(b)
    ints = {4: np.int32, 8: np.int64}[a.dtype.itemsize]
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na].view(ints), b[~nb].view(ints)))


# ------------------------------------------------------------------ 1. the rule
def rule_loop(passes, want, ys, sh, grid, n_scan):
    """The rule, written out per element with scalar arithmetic: ``passes[t][i]`` is the fp32
    prediction of row i in pass t (the first ``n_scan`` passes scan ``grid``, the rest refine)."""
    M = len(want)
    f32, f64 = np.float32, np.float64
    lo, hi, bx, xq = (np.zeros(M, f32) for _ in range(4))
    flo, fhi, br = (np.zeros(M, f64) for _ in range(3))
    status = np.zeros(M, np.int32)
    with np.errstate(all="ignore"):
        for t, p in enumerate(passes):
            for i in range(M):
                r = f64(p[i]) * f64(ys) + f64(sh) - f64(want[i])
                if t == 0:
                    x = f32(grid[0])
                    status[i] = 0
                    lo[i] = hi[i] = bx[i] = x
                    flo[i] = fhi[i] = br[i] = r
                elif t < n_scan:
                    x = f32(grid[t])
                    if status[i] == 0:
                        if abs(r) < abs(br[i]) or (np.isnan(br[i]) and not np.isnan(r)):
                            bx[i], br[i] = x, r
                        if (flo[i] <= 0 and r >= 0) or (flo[i] >= 0 and r <= 0):
                            hi[i], fhi[i], status[i] = x, r, 1
                        else:
                            lo[i] = hi[i] = x
                            flo[i] = fhi[i] = r
                elif status[i] == 1:
                    x = xq[i]
                    same = (r < 0) if flo[i] < 0 else ((r > 0) if flo[i] > 0 else False)
                    if same:
                        lo[i], flo[i] = x, r
                    else:
                        hi[i], fhi[i] = x, r
                xq[i] = f32(lo[i] + f32(f32(hi[i] - lo[i]) * f32(0.5))) if status[i] == 1 else bx[i]
    return np.stack([lo, hi, bx, xq]), np.stack([flo, fhi, br]), status


def planted(m, seed, n_scan=5, n_refine=3, ys=2.0, sh=0.5):
    """Predictions of ``n_scan + n_refine`` passes over m rows and the wanted values: random rows,
    and (from row 0, as far as m reaches) the planted residual sequences. With ys = 2, sh = 0.5 and
    predictions that are multiples of 1/8 the planted residuals are exact."""
    rng = np.random.default_rng(seed)
    T = n_scan + n_refine
    want = (rng.normal(size=m) * 2).astype(np.float32)
    p = ((want[None, :] - sh) / ys + rng.normal(size=(T, m))).astype(np.float32)
    res = [
        [0, 1, 2, 3, 4, -1, 1, -1],          # 0: residual exactly 0 at the first grid point
        [-2, -1, 0, 1, 2, 1, -1, 1],         # 1: ... at a middle one
        [-4, -3, -2, -1, 0, -1, 1, 0],       # 2: ... at the last one (and at a refine pass)
        [-1, 1, -1, 1, 2, -1, -1, 1],        # 3: two crossings: the first wins
        [5, 3, 2, 3, 4, -9, -9, -9],         # 4: no crossing
        [3, 2, 4, 2, 5, 1, 1, 1],            # 5: equal misses: the first wins
        [-3, NAN, -1, 1, 2, 1, NAN, -1],     # 6: NaN at one scan pass (it does not bracket) and at one refine pass
        [NAN, 3, 2, 1, 2, 0, 0, 0],          # 7: NaN first: the first number replaces it
        [NAN] * 8,                           # 8: all NaN
        [2, 1, NAN, -1, 1, 1, 1, 1],         # 9: a NaN between the two sides: no bracket across it
        [0, 0, 0, 0, 0, 0, 0, 0],            # 10: zero everywhere
    ]
    for i, seq in enumerate(res[:m]):
        want[i] = np.float32(3.0)
        p[:, i] = [np.float32((3.0 + v - sh) / ys) for v in seq[:T]]
    return [p[t].copy() for t in range(T)], want


def run_host(passes, want, ys, sh, grid, n_scan):
    from wellflow.setpoint import FIRST, REFINE, SCAN, new_state, solve_step_host

    xs, fs, status = new_state(len(want))
    for t, p in enumerate(passes):
        mode = FIRST if t == 0 else (SCAN if t < n_scan else REFINE)
        solve_step_host(p, want, ys, sh, mode, grid[t] if t < n_scan else None, xs, fs, status)
    return xs, fs, status


GRID5 = np.asarray([1.0, 2.5, 3.0, 7.0, 8.0], np.float32)


@pytest.mark.parametrize("m,ys,sh", [(11, 2.0, 0.5), (1, 2.0, 0.5), (257, 37.25 + 1.0 / 3.0, 101.0 / 7.0)])
def test_numpy_rule_equals_a_per_element_loop(m, ys, sh):
    passes, want = planted(m, 5 + m, ys=2.0, sh=0.5)
    xs, fs, status = run_host(passes, want, ys, sh, GRID5, 5)
    wxs, wfs, wstatus = rule_loop(passes, want, ys, sh, GRID5, 5)
    assert same_bits(xs, wxs) and same_bits(fs, wfs) and same_bits(status, wstatus)
    if (m, ys) != (11, 2.0):
        return
    # the planted rows, by hand
    lo, hi, bx, xq = xs
    flo, fhi, br = fs
    assert status.tolist() == [1, 1, 1, 1, 0, 0, 1, 0, 0, 1, 1]
    assert (lo[0], hi[0], flo[0]) == (1.0, 1.1875, 0.0)          # [x0, x1], then hi moves in: f_lo == 0 is never 'same'
    assert (lo[1], hi[1], fhi[1]) == (2.625, 2.6875, 1.0)        # (x1, x2] with f_hi == 0, refined from both sides
    assert (lo[2], flo[2]) == (7.5, -1.0) and (hi[2], fhi[2]) == (7.625, 0.0)  # 7.5 / 7.75 / 7.625: lo, hi, hi
    assert lo[3] >= 1.0 and hi[3] <= 2.5                          # the first crossing, not the second
    assert (bx[4], br[4], xq[4]) == (3.0, 2.0, 3.0) and lo[4] == hi[4] == 8.0  # nearest: the smallest |r|
    assert (bx[5], br[5]) == (2.5, 2.0)                           # the first of the equal misses
    assert lo[6] >= 3.0 and hi[6] <= 7.0 and np.isnan(fhi[6])     # bracketed after the NaN; the refine NaN lands in f_hi
    assert (bx[7], br[7]) == (7.0, 1.0)                           # the NaN of the first pass is replaced, then improved
    assert np.isnan(fs[:, 8]).all() and (xs[:, 8] == 8.0).sum() == 2 and bx[8] == 1.0
    assert lo[9] >= 7.0 and hi[9] <= 8.0                           # 1 | NaN | -1 does not bracket; -1 | 1 does
    assert (lo[10], hi[10]) == (1.0, np.float32(1.0 + 1.5 / 8))
    from wellflow.setpoint import finish_host

    fin = finish_host(xs, fs, status)
    assert fin["code"].tolist() == [1, 1, 1, 1, 0, 0, 2, 0, 2, 1, 1]
    assert fin["setpoint"][0] == 1.0 and fin["setpoint"][10] == 1.0  # f_lo == f_hi == 0: lo
    assert fin["setpoint"][2] == 7.625 and fin["miss"][2] == 1.0     # the secant ends on the zero
    assert fin["setpoint"][4] == 3.0 and fin["miss"][4] == 2.0
    assert np.isnan(fin["setpoint"][6]) and np.isnan(fin["miss"][8]) and fin["setpoint"][8] == 1.0
    # a NaN stays in its row: the other rows equal a run without it
    clean = [p.copy() for p in passes]
    for p in clean:
        p[[6, 7, 8, 9]] = 1.0
    cxs, cfs, cst = run_host(clean, want, ys, sh, GRID5, 5)
    keep = [0, 1, 2, 3, 4, 5, 10]
    assert same_bits(cxs[:, keep], xs[:, keep]) and same_bits(cfs[:, keep], fs[:, keep])


# ------------------------------------------------------------------ 2. Gilbert: the closed form
def _answerable(cols, column, flow64):
    """The rows of a table whose every row has its answer inside the column's range. A row that
    holds the column's minimum or maximum has its answer AT the end of the grid, and the float32
    cast of its wanted flow (half an ulp either way) decides whether the residual there lies on the
    inner or the outer side of zero; on the outer side the row has no crossing in [min, max], by
    the rule's own definition. Such rows are taken out (the next row is then the end and is looked
    at in turn), read off the closed-form model alone. Every row that is kept must bracket."""
    x = cols[column]
    rising = column != "glr"  # the flow grows with whp and choke and falls with glr
    r = (flow64 - flow64.astype(np.float32).astype(np.float64)) * (1.0 if rising else -1.0)
    keep = np.ones(len(x), bool)
    while True:
        lo, hi = x[keep].min(), x[keep].max()
        bad = keep & (((x == lo) & (r > 0)) | ((x == hi) & (r < 0)))
        if not bad.any():
            return np.flatnonzero(keep)
        keep &= ~bad


@pytest.mark.parametrize("column", ["choke", "whp", "glr"])
def test_gilbert_setpoints_meet_the_closed_form(tmp_path, column):
    from wellflow.models.gilbert import CORRELATIONS, GilbertModel
    from wellflow.predict import Predictor
    from wellflow.setpoint import SetPoint

    table = dict(_synth(3, 80))
    model = GilbertModel(correlation="ros")
    rows = _answerable({k: np.asarray(table[k], np.float64) for k in ("whp", "choke", "glr")}, column,
                       model.predict({k: np.asarray(table[k], np.float64) for k in ("whp", "choke", "glr")}))
    assert 200 <= len(rows) <= 240
    table = take(table, rows)
    n = len(rows)
    p = str(tmp_path / "models" / "gilbert.mdl")
    save_mdl(p, "gilbert", [("Gilbert", [torch.tensor([17.4, 0.5, 2.0])])], {"correlation": "ros", "glr_unit": "scf"})
    cols = {k: np.asarray(table[k], np.float64) for k in ("whp", "choke", "glr")}
    want = model.predict(cols).astype(np.float32)  # the model's own flow of each row
    P, S = 17, 12
    res = SetPoint(Predictor.load(p, _schema(), device="cpu"), points=P, refine=S).run(table, column, want)
    assert res["scored"] == n and not res["native"] and res["passes"] == 1 + P + S
    assert res["grid"][0] == np.float32(cols[column].min()) and res["grid"][-1] == np.float32(cols[column].max())
    assert set(res["status"]) == {"bracketed"} and res["bracketed"] == n and res["open"] == 0  # every row
    A, B, C, unit = CORRELATIONS["ros"]
    assert unit == "scf"
    q, Pw, Sc, R = want.astype(np.float64), cols["whp"], cols["choke"], cols["glr"] * 1000.0
    star = {"choke": (q * A * R ** B / Pw) ** (1.0 / C), "whp": q * A * R ** B / Sc ** C,
            "glr": (Pw * Sc ** C / (A * q)) ** (1.0 / B) / 1000.0}[column]
    step = float(np.max(np.diff(res["grid"].astype(np.float64))))
    bound = step / 2.0 ** S + S * 2.0 ** -24 * np.abs(res["hi"])
    err = np.abs(res["setpoint"] - star)
    print(column, "rows", n, "max |setpoint - S*| / bound", float((err / bound).max()), "median width", res["median_width"])
    assert (err <= bound).all(), float((err / bound).max())
    assert (res["lo"] <= res["setpoint"]).all() and (res["setpoint"] <= res["hi"]).all()


# ------------------------------------------------------------------ 3. a bracket is real
@pytest.fixture(scope="module")
def mlp(tmp_path_factory):
    """A small MLP fitted for a few hundred steps on the synthetic table (8 wells x 125 steps,
    F = 18); its first layer does not read the continuous 'temp'."""
    from wellflow.models.mlp import MLPRegressor

    d = tmp_path_factory.mktemp("setpoint_mlp")
    schema = _schema()
    path, table = _csv_file(d, _synth(8, 125))
    pipe = FeaturePipeline(schema, "flow", standardize_target=True).fit(table)
    assert pipe.n_features == 18 and list(pipe.continuous).index("temp") == 4
    torch.manual_seed(0)
    ref = MLPRegressor(18, (32, 16))
    X = torch.from_numpy(pipe.features(table))
    y = torch.from_numpy(np.asarray(pipe.target_values(table), np.float32)).reshape(-1)
    opt = torch.optim.Adam(ref.parameters(), lr=1e-2)
    for _ in range(300):
        with torch.no_grad():
            ref.linears()[0].weight[:, 11 + 4] = 0.0
        opt.zero_grad()
        loss = ((ref(X).reshape(-1) - y) ** 2).mean()
        loss.backward()
        opt.step()
    with torch.no_grad():
        ref.linears()[0].weight[:, 11 + 4] = 0.0
    sp = str(d) + "/"
    save_mdl(sp + "models/mlp.mdl", "mlp", registry.keras_layers("mlp", ref), {"features": pipe.state()})
    ref.eval()
    return dict(sp=sp, path=path, table=table, pipe=pipe, ref=ref, schema=schema)


def _load(m, name="mlp", **kw):
    from wellflow.predict import Predictor

    return Predictor.load(m["sp"] + f"models/{name}.mdl", m["schema"], device="cpu", precision="fp32", **kw)


def test_rescoring_at_lo_and_hi_gives_f_lo_and_f_hi(mlp):
    from wellflow.scoring import MlpPass, RowValues
    from wellflow.setpoint import SetPoint

    table, pipe = mlp["table"], mlp["pipe"]
    want = np.asarray(table["flow"], np.float32)
    pred = _load(mlp)
    res = SetPoint(pred, points=9, refine=5).run(table, "choke", want)
    assert res["scored"] == 1000 and not res["native"] and res["refine"] == 5 and res["passes"] == 15
    got = res["bracket"] == 1
    assert 100 < got.sum() and res["bracketed"] == int(got.sum()) and res["open"] == 1000 - int(got.sum())
    k = [c for c, _ in SetPoint(pred).input_columns()].index("choke")
    ps = MlpPass(pred, table)
    for end, f in (("lo", "f_lo"), ("hi", "f_hi")):
        p = ps.score(RowValues(k, res[end].astype(np.float32)))
        assert p.dtype == np.float32
        r = p.astype(np.float64) * float(pipe.y_std) + float(pipe.y_mean) - want.astype(np.float64)
        assert same_bits(r[got], res[f][got]), end
    assert (res["lo"][got] <= res["setpoint"][got]).all() and (res["setpoint"][got] <= res["hi"][got]).all()
    assert (np.sign(res["f_lo"][got]) * np.sign(res["f_hi"][got]) <= 0).all()
    width = (res["hi"] - res["lo"])[got]
    step = float(np.diff(res["grid"].astype(np.float64)).max())
    assert (width <= step / 2 ** 5 + 5 * 2.0 ** -24 * np.abs(res["hi"][got])).all()
    assert res["median_width"] == float(np.median(np.abs(width)))
    # the baseline pass is the prediction job's
    assert np.allclose(res["prediction"], pred.predict_table(table), rtol=1e-6, atol=0)
    # a column the model does not read: no row crosses, and the first grid value is the nearest
    flat = SetPoint(pred, points=5, refine=3).run(table, "temp", want)
    assert set(flat["status"]) == {"nearest"} and flat["bracketed"] == 0 and flat["open"] == 1000
    assert (flat["setpoint"] == float(flat["grid"][0])).all()
    assert np.array_equal(flat["miss"], flat["prediction"] - want.astype(np.float64))
    assert np.isnan(flat["median_width"])
    # a scalar want is every row's; --grid order is kept (a descending scan brackets from above)
    one = SetPoint(pred, refine=0).run(table, "choke", 900.0, grid=["60", 40, "20"])
    assert (one["wanted"] == 900.0).all() and one["grid"].tolist() == [60.0, 40.0, 20.0]
    b = one["bracket"] == 1
    assert b.any() and (one["lo"][b] > one["hi"][b]).all()


# ------------------------------------------------------------------ 4. the job: CSV, stdout, dispatch, ranks
def test_job_csv_layout_and_stdout(mlp, tmp_path):
    from wellflow.setpoint import RESULT_COLUMNS, run_setpoint

    sp, path = mlp["sp"], mlp["path"]
    lines = []
    res = run_setpoint("mlp", [NAMES, TYPES, "flow", sp, path, *CPU, "--column", "choke", "--want-column", "flow",
                               "--points", "5", "--refine", "2"], log=lambda s: lines.append(str(s)))
    assert res["out"] == sp + "setpoint/mlp.csv" and not os.path.exists(res["out"] + ".tmp")
    head, rows = _read(res["out"])
    assert head == NAMES.split(",") + TAIL and list(RESULT_COLUMNS) == TAIL and len(rows) == 1000
    flow = np.asarray(mlp["table"]["flow"], np.float32)
    for i in (0, 1, 500, 999):
        r = rows[i]
        assert r[0] == str(mlp["table"]["well"][i])
        assert r[10] == repr(float(res["prediction"][i])) and r[11] == repr(float(flow[i]))
        assert r[12] == repr(float(res["setpoint"][i])) and r[13] == res["status"][i]
        assert r[14] == repr(float(res["lo"][i])) and r[15] == repr(float(res["hi"][i])) and r[16] == repr(float(res["miss"][i]))
    assert {r[13] for r in rows} == {"bracketed", "nearest"}
    assert lines == ["Rows scored: 1000", "Rows bracketed: %d" % res["bracketed"],
                     "Rows without a crossing: %d" % res["open"], "Median bracket width: %f" % res["median_width"]]
    assert res["bracketed"] + res["open"] == 1000 and res["bracketed"] == sum(r[13] == "bracketed" for r in rows)
    # --out, --want, --grid
    out2 = str(tmp_path / "deep" / "sp.csv")
    g = run_setpoint("mlp", [NAMES, TYPES, "flow", sp, path, *CPU, "--column", "whp", "--want", "750", "--grid",
                             "500, 1500,2500", "--refine", "0", "--out", out2], **QUIET)
    head, rows = _read(out2)
    assert g["out"] == out2 and g["grid"].tolist() == [500.0, 1500.0, 2500.0] and {r[11] for r in rows} == {"750.0"}


def test_submit_dispatches_setpoint(tmp_path, capsys):
    from wellflow import submit
    from wellflow.train.job import run_job

    sp = str(tmp_path) + "/"
    run_job("gilbert", [NAMES, TYPES, "flow", sp, "--synth-wells", "2", "--synth-steps", "50"], **QUIET)
    path, table = _csv_file(tmp_path, _synth(2, 50))
    assert submit.main(["setpoint", "gilbert", NAMES, TYPES, "flow", sp, path, "--column", "choke", "--want-column", "flow",
                        "--points", "5", "--refine", "3"]) == 0
    out = capsys.readouterr().out
    assert "Rows scored: 100" in out and "Rows bracketed: " in out and "Rows without a crossing: " in out
    assert "Median bracket width: " in out
    head, rows = _read(sp + "setpoint/gilbert.csv")
    assert head == NAMES.split(",") + TAIL and len(rows) == 100


def test_other_ranks_skip(mlp, tmp_path, monkeypatch):
    from wellflow.setpoint import run_setpoint

    monkeypatch.setenv("RANK", "1")
    out = str(tmp_path / "r1.csv")
    res = run_setpoint("mlp", [NAMES, TYPES, "flow", mlp["sp"], mlp["path"], *CPU, "--column", "choke", "--want", "900",
                               "--out", out], **QUIET)
    assert res.get("skipped") is True and not os.path.exists(out)


# ------------------------------------------------------------------ 5. LSTM
def test_lstm_scans_only_and_wants_at_the_last_row(tmp_path):
    from wellflow.models.lstm import LSTMRegressor
    from wellflow.predict import Predictor
    from wellflow.setpoint import SetPoint, _write_csv

    T, H = 8, 16
    schema = _schema()
    base = _synth(3, 40)
    inter = np.arange(120).reshape(3, 40).T.ravel()  # t0 of every well, t1 of every well, ...
    keep = np.asarray([i for i in inter if not (i // 40 == 2 and i % 40 >= 5)])  # W002: shorter than the window
    _, table = _csv_file(tmp_path, base, order=keep)
    n = len(table["well"])
    assert n == 85
    pipe = FeaturePipeline(schema, "flow").fit(table)  # target left raw: predictions are network outputs
    torch.manual_seed(2)
    ref = LSTMRegressor(pipe.n_features, H)
    p = str(tmp_path / "models" / "lstm.mdl")
    save_mdl(p, "lstm", registry.keras_layers("lstm", ref),
             {"features": pipe.state(), "job": {"seq_len": T, "group_col": "well", "hidden": H}})
    pred = Predictor.load(p, schema, device="cpu", precision="fp32")
    ids = np.unique(np.asarray(table["well"]).astype(str), return_inverse=True)[1]
    order = np.argsort(ids, kind="stable")
    stable = take(table, order)
    starts = np.asarray(window_starts(n, T, ids[order]))
    rows = order[starts + T - 1]
    ref.eval()

    def direct(v):
        t2 = dict(stable)
        if v is not None:
            t2["choke"] = np.full(n, v, np.float32)  # constant over every timestep of every window
        X = pipe.features(t2)
        with torch.no_grad():
            return ref(torch.from_numpy(X[starts[:, None] + np.arange(T)[None, :]])).numpy().reshape(-1)

    base_p = direct(None)
    want = np.full(n, 1e9, np.float32)
    want[rows] = base_p + np.float32(0.01) * np.where(np.arange(66) % 2 == 0, 1, -1)  # a value per window, at its last row
    notes = []
    grid = [20.0, 35.0, 50.0, 64.0]
    res = SetPoint(pred, refine=12, note=notes.append).run(table, "choke", want, grid=grid)
    assert len(notes) == 1 and "scan only" in notes[0] and "--refine is set to 0" in notes[0]
    assert res["refine"] == 0 and res["passes"] == 5 and res["scored"] == 66 and res["n"] == 85
    assert np.array_equal(res["rows"], rows) and np.array_equal(res["wanted"], want[rows].astype(np.float64))
    assert np.allclose(res["prediction"], base_p, rtol=1e-6, atol=1e-7)
    # the state against the per-element loop over the same scorer's constant passes
    from wellflow.scoring import ConstantColumn
    from wellflow.whatif import scorer_for

    scorer = scorer_for(pred, table, "set-point")
    k = [c for c, _ in SetPoint(pred).input_columns()].index("choke")
    passes = [np.array(scorer.predict(ConstantColumn(k, np.float32(v))), copy=True) for v in grid]
    for got, v in zip(passes, grid):
        assert np.allclose(got, direct(np.float32(v)), rtol=1e-5, atol=1e-6)
    wxs, wfs, wst = rule_loop(passes, want[rows], 1.0, 0.0, np.asarray(grid, np.float32), 4)
    assert same_bits(wst, res["bracket"]) and same_bits(wxs[3], res["xq"])
    for name, w in (("lo", wxs[0]), ("hi", wxs[1]), ("best_x", wxs[2]), ("f_lo", wfs[0]), ("f_hi", wfs[1]), ("best_r", wfs[2])):
        assert same_bits(w.astype(np.float64), res[name]), name
    assert set(res["status"]) == {"bracketed", "nearest"}  # the net moves with the choke: some windows cross
    quiet = SetPoint(pred, refine=0, note=notes.append).run(table, "choke", want, grid=grid)
    assert len(notes) == 1 and same_bits(quiet["setpoint"], res["setpoint"])  # refine = 0 asked for: nothing to say
    res["out"] = str(tmp_path / "l.csv")
    _write_csv(res["out"], table, NAMES.split(","), res)
    head, out_rows = _read(res["out"])
    assert head == NAMES.split(",") + TAIL and len(out_rows) == 85
    has = np.zeros(n, bool)
    has[rows] = True
    for i, r in enumerate(out_rows):
        assert (r[10:] != [""] * 7) == bool(has[i])
    m = int(np.flatnonzero(rows == rows[7])[0])
    assert out_rows[rows[7]][12] == repr(float(res["setpoint"][m]))
    with pytest.raises(ValueError, match="shorter than the window"):
        SetPoint(pred).run(take(table, np.arange(15)), "choke", 1.0)


# ------------------------------------------------------------------ 6. refusals
def test_cnn_is_refused_with_the_reason(tmp_path):
    from wellflow.models.cnn import CNN1DRegressor
    from wellflow.setpoint import run_setpoint

    schema = _schema()
    path, table = _csv_file(tmp_path, _synth(2, 100))
    pipe = FeaturePipeline(schema, "flow", standardize_target=True).fit(table)
    ref = CNN1DRegressor(48, 1, 100, 13, 12).init_keras(5)
    sp = str(tmp_path) + "/"
    save_mdl(sp + "models/cnn.mdl", "cnn", registry.keras_layers("cnn", ref), {"features": pipe.state()})
    with pytest.raises(ValueError, match="target's own history.*no input column"):
        run_setpoint("cnn", [NAMES, TYPES, "flow", sp, path, *CPU, "--column", "choke", "--want", "1"], **QUIET)
    assert not os.path.exists(sp + "setpoint/cnn.csv")


def test_errors_name_the_cause(mlp):
    from wellflow.setpoint import SetPoint, run_setpoint

    table = mlp["table"]
    job = SetPoint(_load(mlp))
    args = [NAMES, TYPES, "flow", mlp["sp"], mlp["path"], *CPU]
    with pytest.raises(ValueError, match="column 'well' is categorical.*continuous"):
        run_setpoint("mlp", args + ["--column", "well", "--want", "1"], **QUIET)
    with pytest.raises(ValueError, match="'flow' is the target column"):
        run_setpoint("mlp", args + ["--column", "flow", "--want", "1"], **QUIET)
    with pytest.raises(ValueError, match="unknown column 'nope'"):
        run_setpoint("mlp", args + ["--column", "nope", "--want", "1"], **QUIET)
    with pytest.raises(ValueError, match="no column to search.*--column"):
        run_setpoint("mlp", args + ["--want", "1"], **QUIET)
    with pytest.raises(ValueError, match="--want V .*or --want-column COL.*neither was given"):
        run_setpoint("mlp", args + ["--column", "choke"], **QUIET)
    with pytest.raises(ValueError, match="--want V .*or --want-column COL.*not both"):
        run_setpoint("mlp", args + ["--column", "choke", "--want", "1", "--want-column", "flow"], **QUIET)
    with pytest.raises(ValueError, match="--want 'high' is not a number"):
        run_setpoint("mlp", args + ["--column", "choke", "--want", "high"], **QUIET)
    with pytest.raises(ValueError, match="lacks the --want-column 'pad'"):
        run_setpoint("mlp", args + ["--column", "choke", "--want-column", "pad"], **QUIET)
    with pytest.raises(ValueError, match="--want-column 'well' is not numeric"):
        run_setpoint("mlp", args + ["--column", "choke", "--want-column", "well"], **QUIET)
    with pytest.raises(ValueError, match=r"holds 1 value\(s\): a scan needs at least 2"):
        run_setpoint("mlp", args + ["--column", "choke", "--want", "1", "--grid", "30"], **QUIET)
    with pytest.raises(ValueError, match="grid value 'wide' of the column 'choke' is not a number"):
        run_setpoint("mlp", args + ["--column", "choke", "--want", "1", "--grid", "30,wide"], **QUIET)
    with pytest.raises(ValueError, match="points must be >= 2"):
        run_setpoint("mlp", args + ["--column", "choke", "--want", "1", "--points", "1"], **QUIET)
    with pytest.raises(ValueError, match="refine must be >= 0"):
        run_setpoint("mlp", args + ["--column", "choke", "--want", "1", "--refine", "-1"], **QUIET)
    with pytest.raises(ValueError, match=r"one value per row \(\[1000\]\), got \(999,\)"):
        job.run(table, "choke", np.zeros(999, np.float32))
    with pytest.raises(ValueError, match="must be numbers"):
        job.run(table, "choke", np.asarray(["a"] * 1000))
    with pytest.raises(ValueError, match="ONE column is searched"):
        job.run(table, ["choke", "whp"], 1.0)
    with pytest.raises(ValueError, match="no rows to score"):
        job.run({k: np.asarray(v)[:0] for k, v in table.items()}, "choke", 1.0)
    with pytest.raises(ValueError, match="lacks the input column 'glr'"):
        job.run({k: v for k, v in table.items() if k != "glr"}, "choke", 1.0)
