"""Prediction intervals on the CPU (fp32 oracle engines): the rank rule against a brute-force count,
the numpy rule against a per-element loop bit for bit, the emulated byte select against np.sort, the
coverage property, the per-family semantics, the bands file and the job's CSV / stdout contract
(wellflow/interval.py)."""
import csv
import os
from fractions import Fraction

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
HEADER = ("by", "relative", "alpha", "group", "rows", "rank", "quantile", "source")
NAN, INF = float("nan"), float("inf")


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
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return bool(a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na].view(np.int32), b[~nb].view(np.int32)))


def planted_scores(m, seed):
    """Random non-negative float32 scores with zeros, runs of equal values, inf, NaN and denormals
    planted (as many as fit)."""
    rng = np.random.default_rng(seed)
    s = np.abs(rng.normal(size=m) * 10.0 ** rng.integers(-3, 4, size=m)).astype(np.float32)
    special = [0.0, 0.0, INF, NAN, 1e-42, 3e-45, 7.5, 7.5, 7.5, NAN, INF, 1e-42]
    at = rng.permutation(m)[: len(special)]
    s[at] = np.asarray(special[: len(at)], np.float32)
    return s


# ------------------------------------------------------------------ 1. the rule
def test_rank_rule_equals_a_brute_force_count():
    from wellflow.interval import conformal_rank, make_bands, select_ranks

    for alpha in ("0.01", "0.05", "0.1", "0.2", "0.5"):
        num, den = Fraction(alpha).numerator, Fraction(alpha).denominator
        for n in range(1, 201):
            # the smallest integer k with k >= (n + 1) (1 - alpha), counted up in integers
            k = 0
            while k * den < (n + 1) * (den - num):
                k += 1
            assert conformal_rank(n, alpha) == k, (n, alpha)
    assert conformal_rank(9, "0.1") == 9 and conformal_rank(8, "0.1") == 9  # 9 rows are the fewest for 90 %
    assert conformal_rank(19, "0.05") == 19 and conformal_rank(99, "0.01") == 99
    assert conformal_rank(10 ** 30, "0.1") == 9 * 10 ** 29 + 1  # exact: no float is formed
    assert select_ranks([9, 8, 0, 200], ["0.1", "0.5"]).tolist() == [[8, 4], [0, 4], [0, 0], [180, 100]]
    # k1 > n: the group falls back to the overall band; the overall group itself: +inf, said once
    notes = []
    q_by = np.asarray([[1.0, 2.0], [3.0, 4.0]], np.float32)
    b = make_bands("well", False, ["0.1", "0.5"], ["A", "B"], [9, 8], q_by, 17, np.asarray([5.0, 6.0], np.float32),
                   notes.append)
    rows = [(r["alpha"], r["group"], r["rows"], r["rank"], r["quantile"], r["source"]) for r in b["rows"]]
    assert rows == [("0.1", "", 17, 17, 5.0, "overall"), ("0.1", "A", 9, 9, 1.0, "group"), ("0.1", "B", 8, 9, 5.0, "overall"),
                    ("0.5", "", 17, 9, 6.0, "overall"), ("0.5", "A", 9, 5, 2.0, "group"), ("0.5", "B", 8, 5, 4.0, "group")]
    assert notes == []
    b = make_bands(None, False, ["0.1", "0.05"], ["A"], [3], np.zeros((1, 2), np.float32), 3, np.zeros(2, np.float32),
                   notes.append)
    assert [r["quantile"] for r in b["rows"]] == [INF] * 4 and [r["source"] for r in b["rows"]] == ["overall"] * 4
    assert len(notes) == 1 and "+inf" in notes[0]
    notes.clear()
    make_bands(None, False, ["0.5"], [], [], None, 3, np.asarray([NAN], np.float32), notes.append)
    assert len(notes) == 1 and "NaN" in notes[0]


def _score_loop(p, y, ys, sh, relative, learned):
    out = np.empty(len(p), np.float32)
    for i in range(len(p)):
        if learned:
            v = np.float64(np.float32(p[i])) * np.float64(ys) + np.float64(sh)
            d = v - np.float64(np.float32(y[i]))
        else:
            v = np.float64(p[i])
            d = v - np.float64(y[i])
        with np.errstate(all="ignore"):
            out[i] = np.float32(abs(d) / abs(v)) if relative else np.float32(abs(d))
    return out


def planted_pairs(m, seed, ys, sh):
    """fp32 network outputs and targets: random, with a NaN prediction, a NaN target, an inf
    prediction, v = 0 with and without d = 0, an exactly zero residual and a residual that
    overflows fp32 planted (as many as fit)."""
    rng = np.random.default_rng(seed)
    p = rng.normal(size=m).astype(np.float32)
    y = (p.astype(np.float64) * ys + sh + rng.normal(size=m) * 3).astype(np.float32)
    v0 = np.float32(-sh / ys)  # v = 0 where this is exact
    plant = [(NAN, 1.0), (1.0, NAN), (INF, 1.0), (v0, 2.0), (v0, 0.0), (1.0, np.float32(ys + sh)), (3e38, -3e38)]
    at = rng.permutation(m)[: len(plant)]
    for i, (a, b) in zip(at, plant):
        p[i], y[i] = a, b
    return p, y


def test_numpy_rule_equals_a_python_loop():
    from wellflow.interval import group_quantiles_host, score_host, score_keys, select_host_radix

    for ys, sh in ((2.0, 0.5), (32.0, -4.0), (37.25 + 1.0 / 3.0, 101.0 / 7.0)):
        p, y = planted_pairs(400, 5, ys, sh)
        for relative in (False, True):
            s = score_host(p, y, ys, sh, relative)
            assert s.dtype == np.float32 and same_bits(s, _score_loop(p, y, ys, sh, relative, True))
            assert np.isnan(s).sum() >= 2 and (s[~np.isnan(s)] >= 0).all()
            assert np.isinf(s).sum() >= 1 or ys > 37  # (-sh / ys is exact for the first two scales)
            g = score_host(p.astype(np.float64), y.astype(np.float64), relative=relative, learned=False)
            assert same_bits(g, _score_loop(p, y, 1.0, 0.0, relative, False))
    # v = 0 in relative mode: x / 0 is inf, 0 / 0 NaN; an overflowing residual is inf in float32
    s = score_host(np.asarray([-0.25, -0.25, 3e38], np.float32), np.asarray([2.0, 0.0, -3e38], np.float32), 2.0, 0.5, True)
    assert s[0] == INF and np.isnan(s[1])
    assert score_host(np.asarray([3e38], np.float32), np.asarray([-3e38], np.float32))[0] == INF
    # the keys: NaN last, one pattern for every NaN; key order is np.sort's order
    s = planted_scores(300, 1)
    s[:2] = np.asarray([np.float32(NAN), -np.float32(NAN)])
    k = score_keys(s)
    assert (k[np.isnan(s)] == 0x7FC00000).all() and k.dtype == np.uint32
    assert same_bits(s[np.argsort(k, kind="stable")], np.sort(s))
    # quantiles per group against a per-element selection, a group of one row and an empty group
    ids = np.random.default_rng(2).integers(0, 5, size=300)
    ids[ids == 3] = 1
    ids[7] = 3  # one row
    ids[ids == 4] = 0  # group 4 is empty
    ranks = np.asarray([[0, 10], [5, 10 ** 6], [1, 2], [0, 0], [0, 0]], np.int32)
    q = group_quantiles_host(s, ids, 5, ranks)
    for g in range(5):
        mine = sorted((float(v) for v in s[ids == g]), key=lambda v: (v != v, v))
        for a in range(2):
            want = mine[min(ranks[g, a], len(mine) - 1)] if mine else NAN
            assert same_bits(q[g, a], np.float32(want)), (g, a)
    assert same_bits(q[3], [s[7], s[7]]) and np.isnan(q[4]).all()
    assert select_host_radix(s[:0], 0) != select_host_radix(s[:0], 0)  # NaN without scores


def test_byte_select_equals_np_sort():
    from wellflow.interval import select_host_radix

    for seed in range(40):
        m = [1, 2, 63, 257, 1000][seed % 5]
        s = planted_scores(m, seed)
        if seed % 7 == 0:
            s[:] = s[0] if s[0] == s[0] else 1.5  # all equal
        if seed % 11 == 0:
            s[:] = np.float32(NAN)
        if seed % 13 == 0:  # scores that differ in one byte of the key only
            base = np.float32(1.0).view(np.uint32)
            s = (base + (np.arange(m, dtype=np.uint32) % 64 << np.uint32(8 * (seed % 4)))).astype(np.uint32).view(np.float32)
        want = np.sort(s)
        for k in sorted({0, m - 1, m // 2, m // 3, -5, m + 5}):
            assert same_bits(select_host_radix(s, k), want[min(max(k, 0), m - 1)]), (seed, k)


def test_coverage_on_the_calibration_rows():
    from wellflow.interval import conformal_rank, group_quantiles_host, score_host, select_ranks

    rng = np.random.default_rng(9)
    m = 700
    p = rng.normal(size=m).astype(np.float32)
    y = (p * 2 + 0.5 + rng.standard_t(3, size=m)).astype(np.float32)
    ids = rng.integers(0, 6, size=m)
    ids[ids == 5] = rng.integers(0, 2, size=(ids == 5).sum()) * 5  # group 5 is small
    counts = np.bincount(ids, minlength=6)
    alphas = ["0.01", "0.1", "0.5"]
    for relative in (False, True):
        s = score_host(p, y, 2.0, 0.5, relative)
        q = group_quantiles_host(s, ids, 6, select_ranks(counts, alphas))
        own = 0
        for g in range(6):
            for a, alpha in enumerate(alphas):
                k1 = conformal_rank(counts[g], alpha)
                if k1 > counts[g]:
                    continue
                own += 1
                covered = int((s[ids == g] <= q[g, a]).sum())
                assert covered >= k1 and covered >= (1 - float(alpha)) * counts[g], (g, alpha)
        assert own > 12


# ------------------------------------------------------------------ 2. the families
@pytest.fixture(scope="module")
def mlp(tmp_path_factory):
    """An MLP with drawn weights on the synthetic table (8 wells x 125 steps, F = 18)."""
    from wellflow.models.mlp import MLPRegressor

    d = tmp_path_factory.mktemp("interval_mlp")
    schema = _schema()
    path, table = _csv_file(d, _synth(8, 125))
    pipe = FeaturePipeline(schema, "flow", standardize_target=True).fit(table)
    torch.manual_seed(0)
    ref = MLPRegressor(18, (32, 16))
    sp = str(d) + "/"
    save_mdl(sp + "models/mlp.mdl", "mlp", registry.keras_layers("mlp", ref), {"features": pipe.state()})
    ref.eval()
    return dict(sp=sp, path=path, table=table, pipe=pipe, ref=ref, schema=schema)


def _load(m, name="mlp", **kw):
    from wellflow.predict import Predictor

    return Predictor.load(m["sp"] + f"models/{name}.mdl", m["schema"], device="cpu", precision="fp32", **kw)


def test_mlp_bands_equal_direct_numpy(mlp):
    from wellflow.interval import ConformalBands, conformal_rank

    table, pipe, ref = mlp["table"], mlp["pipe"], mlp["ref"]
    with torch.no_grad():
        p = ref(torch.from_numpy(pipe.features(table))).numpy().reshape(-1)
    y32 = np.asarray(table["flow"], np.float32)
    groups, ids = np.unique(np.asarray(table["well"]).astype(str), return_inverse=True)
    for relative in (False, True):
        v = p.astype(np.float64) * pipe.y_std + pipe.y_mean
        d = np.abs(v - y32.astype(np.float64))
        s = (d / np.abs(v) if relative else d).astype(np.float32)
        bands = ConformalBands(_load(mlp), alphas=("0.1", "0.05"), by="well", relative=relative).calibrate(table)
        assert bands["scored"] == 1000 and not bands["native"] and bands["groups"] == list(groups)
        assert bands["by"] == "well" and bands["relative"] is relative and bands["alphas"] == ["0.1", "0.05"]
        assert len(bands["rows"]) == 2 * 9
        for a, alpha in enumerate(("0.1", "0.05")):
            blk = bands["rows"][9 * a : 9 * a + 9]
            assert [r["group"] for r in blk] == [""] + list(groups) and all(r["alpha"] == alpha for r in blk)
            assert blk[0]["quantile"] == float(np.sort(s)[conformal_rank(1000, alpha) - 1]) and blk[0]["rows"] == 1000
            for g, r in enumerate(blk[1:]):
                k1 = conformal_rank(125, alpha)
                assert (r["rows"], r["rank"], r["source"]) == (125, k1, "group")
                assert r["quantile"] == float(np.sort(s[ids == g])[k1 - 1])
    # applied: the prediction job's value, the band of the row's own group, the coverage on these rows
    job = ConformalBands(_load(mlp), alphas=("0.1", "0.05"), by="well")
    bands = job.calibrate(table)
    res = job.apply(table, bands)
    pv = np.asarray(_load(mlp).predict_table(table))
    assert res["scored"] == 1000 and res["unscored"] == 0 and res["levels"] == ["90", "95"]
    assert np.array_equal(res["prediction"], pv) and pv.dtype == np.float32
    for a in range(2):
        q = np.asarray([bands["rows"][9 * a + 1 + g]["quantile"] for g in ids])
        assert np.array_equal(res["lower"][a], pv.astype(np.float64) - q)
        assert np.array_equal(res["upper"][a], pv.astype(np.float64) + q)
        assert res["coverage"][a] >= 1 - float(bands["alphas"][a])
    assert (res["band"] == "group").all()
    rel = ConformalBands(_load(mlp), by="well", relative=True)
    rb = rel.calibrate(table)
    rr = rel.apply(table, rb)
    q = np.asarray([rb["rows"][1 + g]["quantile"] for g in ids])
    assert np.array_equal(rr["upper"][0], pv.astype(np.float64) + q * np.abs(pv.astype(np.float64)))
    # a group the bands do not know, and a group without its own band, take the overall band
    few = take(table, np.flatnonzero((ids != 7) | (np.arange(1000) % 125 < 5)))  # W007: 5 rows, no 90 % band
    fb = ConformalBands(_load(mlp), by="well").calibrate(few)
    w7 = fb["rows"][8]
    assert (w7["group"], w7["rows"], w7["rank"], w7["source"], w7["quantile"]) == ("W007", 5, 6, "overall", fb["rows"][0]["quantile"])
    t2 = dict(table)
    t2["well"] = np.where(ids == 0, "W999", np.asarray(table["well"]).astype(str)).astype(object)
    r2 = ConformalBands(_load(mlp)).apply(t2, fb)
    assert set(r2["band"][ids == 0]) == {"overall"} and set(r2["band"][ids == 7]) == {"overall"} and set(r2["band"][ids == 3]) == {"group"}
    assert np.array_equal(r2["upper"][0][ids == 0], r2["prediction"].astype(np.float64)[ids == 0] + fb["rows"][0]["quantile"])
    # levels that differ in their source: per level, joined
    mixed = ConformalBands(_load(mlp), alphas=("0.5", "0.1"), by="well")
    r3 = mixed.apply(table, mixed.calibrate(few))
    assert set(r3["band"][ids == 7]) == {"group/overall"} and set(r3["band"][ids == 1]) == {"group"}


def test_gilbert_over_the_synthetic_table(tmp_path):
    from wellflow.interval import ConformalBands, conformal_rank
    from wellflow.models.gilbert import GilbertModel
    from wellflow.predict import Predictor

    table = dict(_synth(2, 60))
    p = str(tmp_path / "models" / "gilbert.mdl")
    save_mdl(p, "gilbert", [("Gilbert", [torch.tensor([17.4, 0.5, 2.0])])], {"correlation": "ros", "glr_unit": "scf"})
    job = ConformalBands(Predictor.load(p, _schema(), device="cpu"), alphas=("0.2",), by="well")
    with pytest.raises(ValueError, match="gilbert: name the target column"):
        job.calibrate(table)
    bands = job.calibrate(table, target="flow")
    v = GilbertModel(correlation="ros").predict({k: np.asarray(table[k], np.float64) for k in ("whp", "choke", "glr")})
    s = np.abs(v - np.asarray(table["flow"], np.float64)).astype(np.float32)
    ids = np.unique(np.asarray(table["well"]).astype(str), return_inverse=True)[1]
    assert bands["scored"] == 120 and not bands["native"]
    assert bands["rows"][0]["quantile"] == float(np.sort(s)[conformal_rank(120, "0.2") - 1])
    assert [r["quantile"] for r in bands["rows"][1:]] == [float(np.sort(s[ids == g])[conformal_rank(60, "0.2") - 1]) for g in (0, 1)]
    res = job.apply(table, bands, target="flow")
    assert res["prediction"].dtype == np.float64 and np.array_equal(res["prediction"], v)
    assert res["coverage"][0] >= 0.8 and job.apply(table, bands)["coverage"] is None


def test_lstm_group_and_target_at_the_last_row(tmp_path):
    from wellflow.interval import ConformalBands, conformal_rank, run_interval
    from wellflow.models.lstm import LSTMRegressor
    from wellflow.predict import Predictor

    T, H = 8, 16
    schema = _schema()
    base = _synth(3, 40)
    inter = np.arange(120).reshape(3, 40).T.ravel()  # t0 of every well, t1 of every well, ...
    keep = np.asarray([i for i in inter if not (i // 40 == 2 and i % 40 >= 5)])  # W002: 5 rows, no window
    path, table = _csv_file(tmp_path, base, order=keep)
    n = len(table["well"])
    pipe = FeaturePipeline(schema, "flow").fit(table)  # target left raw
    torch.manual_seed(2)
    ref = LSTMRegressor(pipe.n_features, H)
    sp = str(tmp_path) + "/"
    save_mdl(sp + "models/lstm.mdl", "lstm", registry.keras_layers("lstm", ref),
             {"features": pipe.state(), "job": {"seq_len": T, "group_col": "well", "hidden": H}})
    pred = Predictor.load(sp + "models/lstm.mdl", schema, device="cpu", precision="fp32")
    bands = ConformalBands(pred, alphas=("0.2",), by="well").calibrate(table)
    ids = np.unique(np.asarray(table["well"]).astype(str), return_inverse=True)[1]
    order = np.argsort(ids, kind="stable")
    stable = take(table, order)
    starts = np.asarray(window_starts(n, T, ids[order]))
    last = starts + T - 1
    X = pipe.features(stable)
    ref.eval()
    with torch.no_grad():
        p = ref(torch.from_numpy(X[starts[:, None] + np.arange(T)[None, :]])).numpy().reshape(-1)
    s = np.abs(p.astype(np.float64) - np.asarray(stable["flow"], np.float32)[last].astype(np.float64)).astype(np.float32)
    wid = ids[order][last]
    assert bands["scored"] == 66 and [r["rows"] for r in bands["rows"]] == [66, 33, 33, 0]
    assert bands["rows"][0]["quantile"] == float(np.sort(s)[conformal_rank(66, "0.2") - 1])
    for g in (0, 1):
        assert bands["rows"][1 + g]["quantile"] == float(np.sort(s[wid == g])[conformal_rank(33, "0.2") - 1])
    assert (bands["rows"][3]["source"], bands["rows"][3]["rank"], bands["rows"][3]["quantile"]) == \
        ("overall", 1, bands["rows"][0]["quantile"])
    # the job: empty cells for the first T - 1 rows of each series (and all of W002)
    args = [NAMES, TYPES, "flow", sp, path, *CPU]
    run_interval("lstm", args + ["--calibrate", "--alpha", "0.2", "--by", "well"], **QUIET)
    lines = []
    res = run_interval("lstm", args, log=lambda s: lines.append(str(s)))
    head, rows = _read(res["out"])
    assert head == NAMES.split(",") + ["prediction", "lower_80", "upper_80", "band"] and len(rows) == n
    seen = {}
    for r in rows:
        k = seen[r[0]] = seen.get(r[0], 0) + 1
        if k < T or r[0] == "W002":
            assert r[10:] == ["", "", "", ""]
        else:
            assert r[13] == "group" and float(r[11]) < float(r[10]) < float(r[12])
    assert lines[:2] == ["Rows scored: 66", "Rows without prediction: 19"] and lines[2].startswith("Empirical coverage 80: ")
    assert res["coverage"][0] >= 0.8


# ------------------------------------------------------------------ 3. the bands file and the job
def test_bands_file_round_trip_and_layout(tmp_path):
    from wellflow.interval import BANDS_COLUMNS, read_bands, write_bands

    q = [float(np.float32(0.1)), float(np.float32(1e-42)), INF, NAN, 0.0, float(np.float32(123456.789))]
    rows = [{"alpha": "0.1", "group": "", "rows": 40, "rank": 37, "quantile": q[0], "source": "overall"},
            {"alpha": "0.1", "group": "a,b", "rows": 30, "rank": 28, "quantile": q[1], "source": "group"},
            {"alpha": "0.1", "group": "c", "rows": 10, "rank": 10, "quantile": q[2], "source": "group"},
            {"alpha": "0.05", "group": "", "rows": 40, "rank": 39, "quantile": q[3], "source": "overall"},
            {"alpha": "0.05", "group": "a,b", "rows": 30, "rank": 30, "quantile": q[4], "source": "group"},
            {"alpha": "0.05", "group": "c", "rows": 10, "rank": 11, "quantile": q[5], "source": "overall"}]
    bands = {"by": "well", "relative": True, "alphas": ["0.1", "0.05"], "groups": ["a,b", "c"], "rows": rows}
    path = str(tmp_path / "deep" / "b.csv")
    write_bands(path, bands)
    assert not os.path.exists(path + ".tmp")
    head, cells = _read(path)
    assert tuple(head) == BANDS_COLUMNS == HEADER
    assert cells[0] == ["well", "1", "0.1", "", "40", "37", repr(q[0]), "overall"]
    assert cells[1] == ["well", "1", "0.1", "a,b", "30", "28", repr(q[1]), "group"]
    assert [c[6] for c in cells[2:5]] == ["inf", "nan", "0.0"]
    back = read_bands(path)
    assert {k: back[k] for k in ("by", "relative", "alphas", "groups")} == {k: bands[k] for k in ("by", "relative", "alphas", "groups")}
    for r, w in zip(back["rows"], rows):
        assert {k: r[k] for k in r if k != "quantile"} == {k: w[k] for k in w if k != "quantile"}
        assert same_bits(np.float32(r["quantile"]), np.float32(w["quantile"])) and (r["quantile"] == w["quantile"] or w["quantile"] != w["quantile"])


def test_job_calibrate_then_apply(mlp, tmp_path, capsys):
    from wellflow import submit
    from wellflow.interval import run_interval

    sp, path = mlp["sp"], mlp["path"]
    args = [NAMES, TYPES, "flow", sp, path, *CPU]
    lines = []
    cal = run_interval("mlp", args + ["--calibrate", "--alpha", "0.1,0.05", "--by", "well"], log=lambda s: lines.append(str(s)))
    assert cal["out"] == sp + "interval/mlp.bands.csv" and not os.path.exists(sp + "interval/mlp.csv")
    head, cells = _read(cal["out"])
    assert tuple(head) == HEADER and len(cells) == 18 and [c[3] for c in cells[:2]] == ["", "W000"]
    assert lines == ["Calibration rows scored: 1000", "Overall quantile 90: %f" % cal["rows"][0]["quantile"],
                     "Overall quantile 95: %f" % cal["rows"][9]["quantile"]]
    lines.clear()
    res = run_interval("mlp", args, log=lambda s: lines.append(str(s)))
    assert res["out"] == sp + "interval/mlp.csv" and not os.path.exists(res["out"] + ".tmp")
    head, rows = _read(res["out"])
    assert head == NAMES.split(",") + ["prediction", "lower_90", "upper_90", "lower_95", "upper_95", "band"]
    assert len(rows) == 1000 and rows[0][:2] == ["W000", str(mlp["table"]["field"][0])]
    for i in (0, 517, 999):
        assert rows[i][10] == repr(float(res["prediction"][i])) and rows[i][13] == repr(float(res["lower"][1][i]))
        assert float(rows[i][13]) <= float(rows[i][11]) < float(rows[i][10]) < float(rows[i][12]) <= float(rows[i][14])
        assert rows[i][15] == "group"
    assert lines == ["Rows scored: 1000", "Rows without prediction: 0", "Empirical coverage 90: %f" % res["coverage"][0],
                     "Empirical coverage 95: %f" % res["coverage"][1]]
    assert res["coverage"][0] >= 0.9 and res["coverage"][1] >= 0.95
    # the default level, --bands and --out; no --by: only the overall band
    b2, o2 = str(tmp_path / "x" / "b.csv"), str(tmp_path / "y" / "o.csv")
    cal = run_interval("mlp", args + ["--calibrate", "--relative", "--bands", b2], **QUIET)
    assert cal["out"] == b2 and _read(b2)[1] == [["", "1", "0.1", "", "1000", "901", repr(cal["rows"][0]["quantile"]), "overall"]]
    res = run_interval("mlp", args + ["--bands", b2, "--out", o2], **QUIET)
    head, rows = _read(o2)
    assert head[10:] == ["prediction", "lower_90", "upper_90", "band"] and {r[13] for r in rows} == {"overall"}
    # submit interval
    assert submit.main(["interval", "mlp", *args, "--calibrate", "--bands", b2]) == 0
    assert submit.main(["interval", "mlp", *args, "--bands", b2, "--out", o2]) == 0
    out = capsys.readouterr().out
    assert "Calibration rows scored: 1000" in out and "Empirical coverage 90: " in out


def test_other_ranks_skip(mlp, tmp_path, monkeypatch):
    from wellflow.interval import run_interval

    monkeypatch.setenv("RANK", "1")
    b, o = str(tmp_path / "b.csv"), str(tmp_path / "o.csv")
    args = [NAMES, TYPES, "flow", mlp["sp"], mlp["path"], *CPU, "--bands", b, "--out", o]
    assert run_interval("mlp", args + ["--calibrate"], **QUIET).get("skipped") is True
    assert run_interval("mlp", args, **QUIET).get("skipped") is True
    assert not os.path.exists(b) and not os.path.exists(o)


# ------------------------------------------------------------------ 4. refusals
def test_cnn_is_refused_with_the_reason(tmp_path):
    from wellflow.interval import run_interval
    from wellflow.models.cnn import CNN1DRegressor

    schema = _schema()
    path, table = _csv_file(tmp_path, _synth(2, 100))
    pipe = FeaturePipeline(schema, "flow", standardize_target=True).fit(table)
    ref = CNN1DRegressor(48, 1, 100, 13, 12).init_keras(5)
    sp = str(tmp_path) + "/"
    save_mdl(sp + "models/cnn.mdl", "cnn", registry.keras_layers("cnn", ref), {"features": pipe.state()})
    with pytest.raises(ValueError, match="O horizons per window.*band per horizon is not built"):
        run_interval("cnn", [NAMES, TYPES, "flow", sp, path, *CPU, "--calibrate"], **QUIET)
    assert not os.path.exists(sp + "interval/cnn.bands.csv")


def test_errors_name_the_cause(mlp, tmp_path):
    from wellflow.interval import ConformalBands, read_bands, run_interval

    table = mlp["table"]
    args = [NAMES, TYPES, "flow", mlp["sp"], mlp["path"], *CPU]
    b = str(tmp_path / "b.csv")
    cal = args + ["--calibrate", "--bands", b]
    with pytest.raises(ValueError, match="lacks the --by column 'pad'"):
        run_interval("mlp", cal + ["--by", "pad"], **QUIET)
    with pytest.raises(ValueError, match="5 levels: give 1 to 4"):
        run_interval("mlp", cal + ["--alpha", "0.1,0.2,0.3,0.4,0.5"], **QUIET)
    for bad in ("0", "1", "1.5", "-0.1"):
        with pytest.raises(ValueError, match="outside \\(0, 1\\)"):
            run_interval("mlp", cal + ["--alpha=" + bad], **QUIET)
    with pytest.raises(ValueError, match="level 'ten' is not a decimal number"):
        run_interval("mlp", cal + ["--alpha", "ten"], **QUIET)
    with pytest.raises(ValueError, match="level '0.10' is given twice"):
        run_interval("mlp", cal + ["--alpha", "0.1,0.10"], **QUIET)
    assert not os.path.exists(b)
    # calibration without a numeric target
    with pytest.raises(ValueError, match="lacks the target column 'flow'"):
        ConformalBands(_load(mlp)).calibrate({k: v for k, v in table.items() if k != "flow"})
    t2 = dict(table)
    t2["flow"] = np.asarray(["high"] * 1000, dtype=object)
    with pytest.raises(ValueError, match="'flow' is not numeric: a calibration needs a numeric target"):
        ConformalBands(_load(mlp)).calibrate(t2)
    with pytest.raises(ValueError, match="no rows to score"):
        ConformalBands(_load(mlp)).calibrate({k: np.asarray(v)[:0] for k, v in table.items()})
    with pytest.raises(ValueError, match="lacks the input column 'glr'"):
        ConformalBands(_load(mlp)).calibrate({k: v for k, v in table.items() if k != "glr"})
    big = {k: np.tile(np.asarray(v), 9) for k, v in table.items()}
    big["t"] = np.arange(9000)
    with pytest.raises(ValueError, match="9000 groups; with 2 level\\(s\\) at most 8192"):
        ConformalBands(_load(mlp), alphas=("0.1", "0.2"), by="t").calibrate(big)
    # applying: no bands file, options that belong to the calibration, a file that does not parse
    with pytest.raises(FileNotFoundError, match="no bands file at .*calibrate first"):
        run_interval("mlp", args + ["--bands", b], **QUIET)
    for opt, name in ((["--alpha", "0.1"], "--alpha"), (["--by", "well"], "--by"), (["--relative"], "--relative")):
        with pytest.raises(ValueError, match=name + " given without --calibrate: .* read from the bands file"):
            run_interval("mlp", args + ["--bands", b] + opt, **QUIET)
    run_interval("mlp", cal + ["--by", "well"], **QUIET)
    good = open(b).read()
    ln = good.splitlines()

    def edited(i, cell, text, drop=False):
        """The file with cell ``cell`` of line ``i`` (1-based) replaced by ``text`` or dropped."""
        c = ln[i - 1].split(",")
        c = c[:cell] + ([] if drop else [text]) + c[cell + 1 :]
        return "\n".join(ln[: i - 1] + [",".join(c)] + ln[i:]) + "\n"

    broken = {"its header is not": edited(1, 0, "per"),
              "it holds no band": ln[0] + "\n",
              "line 3 has 7 cells": edited(3, 4, "", drop=True),
              "line 2: .*could not convert": edited(2, 6, "wide"),
              "line 4: source 'own'": edited(4, 7, "own"),
              "line 2: .*outside \\(0, 1\\)": edited(2, 2, "1.1"),
              "line 2: level 0.1 does not begin with its overall row": "\n".join(ln[:1] + ln[2:]) + "\n",
              "line 5: 'by' / 'relative' must be the same": edited(5, 0, "field")}
    for why, text in broken.items():
        assert text != good, why
        with open(b, "w") as f:
            f.write(text)
        with pytest.raises(ValueError, match="does not parse: " + why):
            read_bands(b)
    with open(b, "w") as f:
        f.write(good)
    with pytest.raises(ValueError, match="the bands are per 'well' .*which the data lacks"):
        ConformalBands(_load(mlp)).apply({k: v for k, v in table.items() if k != "well"}, read_bands(b))
