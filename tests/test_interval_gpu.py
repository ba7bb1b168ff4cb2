"""Prediction intervals on the GPU: the scores (csrc/quantile.hip abs_scores) and the per-group order
statistics (group_quantiles) against the numpy rule bit for bit, the host-side refusals, and the
native calibration of wellflow/interval.py against the numpy rule over the engine's own
predictions."""
import csv

import numpy as np
import pytest
import torch

from wellflow.data.features import FeaturePipeline, take
from wellflow.data.io import load_table, write_csv
from wellflow.data.schema import parse_schema
from wellflow.models import registry
from wellflow.utils.checkpoint import save_mdl

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0) if torch.cuda.is_available() else None

NAMES = "well,field,t,whp,choke,glr,temp,water_cut,dsp,flow"
TYPES = "string,string,int,float,float,float,float,float,float,float"
QUIET = dict(log=lambda *a, **k: None)
NAN, INF = float("nan"), float("inf")
SIZES = [1, 63, 257, 70001]


def same_bits(a, b):
    """Equal bit for bit where neither is NaN, and NaN at the same positions."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return bool(a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na].view(np.int32), b[~nb].view(np.int32)))


# ------------------------------------------------------------------ 1. abs_scores
def planted_pairs(m, seed, ys, sh):
    """fp32 network outputs and targets: random, with a NaN prediction, a NaN target, an inf
    prediction, v = 0 with and without d = 0, an exactly zero residual and a residual whose fp64
    value overflows fp32 planted (as many as fit)."""
    rng = np.random.default_rng(seed)
    p = rng.normal(size=m).astype(np.float32)
    y = (p.astype(np.float64) * ys + sh + rng.normal(size=m) * 3).astype(np.float32)
    v0 = np.float32(-sh / ys)  # v = 0 where this is exact
    plant = [(3e38, -3e38), (NAN, 1.0), (v0, 2.0), (INF, 1.0), (v0, 0.0), (1.0, NAN), (1.0, np.float32(ys + sh))]
    at = rng.permutation(m)[: len(plant)]
    for i, (a, b) in zip(at, plant):
        p[i], y[i] = a, b
    return p, y


@pytest.mark.parametrize("m", SIZES)
def test_abs_scores_equal_the_numpy_rule(m):
    from wellflow.interval import score_host
    from wellflow.ops.native import abs_scores

    for ys, sh in ((2.0, 0.5), (37.25 + 1.0 / 3.0, 101.0 / 7.0)):
        p, y = planted_pairs(m, m, ys, sh)
        pd, yd = torch.from_numpy(p).to(DEV), torch.from_numpy(y).to(DEV)
        for relative in (False, True):
            buf = torch.full((m + 1,), NAN, dtype=torch.float32, device=DEV)
            spare = buf[m:].view(torch.int32).clone()
            abs_scores(pd, yd, ys, sh, relative, buf[:m])
            got = buf.cpu().numpy()
            want = score_host(p, y, ys, sh, relative)
            assert same_bits(got[:m], want), (ys, relative)
            assert torch.equal(buf[m:].view(torch.int32), spare)  # the element past M is untouched
            if m >= 63 and ys == 2.0:
                assert np.isinf(want).any() and np.isnan(want).any()


# ------------------------------------------------------------------ 2. group_quantiles
def planted_scores(m, seed):
    """Random non-negative float32 scores with zeros, runs of equal values, inf and denormals
    planted (as many as fit); no NaN."""
    rng = np.random.default_rng(seed)
    s = np.abs(rng.normal(size=m) * 10.0 ** rng.integers(-3, 4, size=m)).astype(np.float32)
    special = [0.0, 0.0, INF, 1e-42, 3e-45, 7.5, 7.5, 7.5, INF, 1e-42]
    at = rng.permutation(m)[: len(special)]
    s[at] = np.asarray(special[: len(at)], np.float32)
    return s


def _ranks(counts, A):
    """int32 [G][A]: the middle (A = 1); the first, the last, the middle and the middle again (A = 4)."""
    n = np.maximum(np.asarray(counts, np.int64), 1)
    cols = [n // 2] if A == 1 else [0 * n, n - 1, n // 2, n // 2]
    return np.stack(cols, axis=1).astype(np.int32)



def select_device(s, ids, G, ranks, pad=5):
    """(quantiles [G][A], the plan): ``out`` is a NaN-prefilled buffer ``pad`` elements longer than
    [G][A] whose tail must stay as it was."""
    from wellflow.ops.native import QuantilePlan, group_quantiles

    A = ranks.shape[1]
    plan = QuantilePlan(ids, G, A, DEV)
    buf = torch.full((G * A + pad,), NAN, dtype=torch.float32, device=DEV)
    group_quantiles(torch.from_numpy(s).to(DEV), plan, torch.from_numpy(ranks).to(DEV), buf[: G * A].view(G, A))
    assert bool(torch.isnan(buf[G * A :]).all()), "group_quantiles wrote outside out"
    assert not bool(plan.hist.any()), "hist is not left zero"
    return buf[: G * A].view(G, A).cpu().numpy(), plan


@pytest.mark.parametrize("m", SIZES)
def test_group_quantiles_equal_np_sort(m):
    from wellflow.interval import group_quantiles_host
    from wellflow.ops.native import group_quantiles

    s = planted_scores(m, m)
    for G in (1, 3, 1000):
        rng = np.random.default_rng(G + m)
        for layout in ("random", "sorted"):
            ids = rng.integers(0, G, size=m)
            if G == 3 and m > 3:
                ids[ids == 1] = 2  # group 1 is empty
            if layout == "sorted":
                ids = np.sort(ids)
            counts = np.bincount(ids, minlength=G)
            for A in (1, 4):
                ranks = _ranks(counts, A)
                got, plan = select_device(s, ids, G, ranks)
                want = group_quantiles_host(s, ids, G, ranks)
                assert same_bits(got, want), (G, layout, A)
                assert np.isnan(got[counts == 0]).all() and not np.isnan(got[counts > 0]).any()
                if A == 4:
                    assert same_bits(got[:, 2], got[:, 3])  # two equal ranks
                # a second call on the same plan: bitwise equal, hist zero again
                out2 = torch.full((G, A), NAN, dtype=torch.float32, device=DEV)
                group_quantiles(torch.from_numpy(s).to(DEV), plan, torch.from_numpy(ranks).to(DEV), out2)
                assert same_bits(out2.cpu().numpy(), got) and not bool(plan.hist.any())
        # a NaN score reaches its own group only (it sorts last there)
        if G > 1 and m >= 63:
            ids = rng.integers(0, G, size=m)
            ids[:2] = 0
            ranks = _ranks(np.bincount(ids, minlength=G), 4)
            clean, _ = select_device(s, ids, G, ranks)
            s2 = s.copy()
            s2[0] = NAN
            dirty, _ = select_device(s2, ids, G, ranks)
            assert same_bits(dirty[1:], clean[1:]) and np.isnan(dirty[0, 1]) and not np.isnan(clean[0, 1])
            assert same_bits(dirty, group_quantiles_host(s2, ids, G, ranks))


def byte_scores(n, byte):
    """n scores whose keys differ only in one byte (3: the most significant)."""
    base = np.float32(1.0).view(np.uint32)
    step = np.random.default_rng(byte).integers(0, 64, size=n).astype(np.uint32)
    return (base + (step << np.uint32(8 * byte))).astype(np.uint32).view(np.float32)


PLANTED = {
    "equal": lambda n: np.full(n, 7.5, np.float32),
    "byte3": lambda n: byte_scores(n, 3),
    "byte2": lambda n: byte_scores(n, 2),
    "byte1": lambda n: byte_scores(n, 1),
    "byte0": lambda n: byte_scores(n, 0),
    "denormal": lambda n: (np.random.default_rng(1).integers(0, 2 ** 23, size=n).astype(np.uint32)).view(np.float32),
    "nan": lambda n: np.full(n, NAN, np.float32),
}


@pytest.mark.parametrize("what", list(PLANTED))
def test_group_quantiles_planted_keys(what):
    """Group sizes at the piece boundaries (a piece holds 1024 positions), one small launch."""
    from wellflow.interval import group_quantiles_host

    sizes = [1, 1023, 1024, 1025, 2049]
    ids = np.random.default_rng(3).permutation(np.repeat(np.arange(5), sizes))
    s = PLANTED[what](len(ids))
    assert (s[~np.isnan(s)] >= 0).all()
    ranks = _ranks(sizes, 4)
    ranks[:, 3] = np.minimum(np.asarray(sizes) - 1, 1023)  # the last position of the first piece
    got, _ = select_device(s, ids, 5, ranks)
    assert same_bits(got, group_quantiles_host(s, ids, 5, ranks)), what
    if what == "nan":
        assert np.isnan(got).all()
    elif what != "equal":
        assert (got[4, 0] < got[4, 1]) and got[4, 0] <= got[4, 2] <= got[4, 1]
    # ranks outside a group are clamped into it
    wild = np.asarray([[-7, 10 ** 6, 2 ** 31 - 1, -2 ** 31]] * 5, np.int32)
    got, _ = select_device(s, ids, 5, wild)
    assert same_bits(got, group_quantiles_host(s, ids, 5, wild)), what


def test_refusals_come_from_the_host():
    from wellflow.ops.native import QuantilePlan, abs_scores, group_quantiles, lib

    m = 10
    p, y = torch.zeros(m, device=DEV), torch.ones(m, device=DEV)
    out = torch.full((m,), 7.0, device=DEV)
    with pytest.raises(TypeError, match="pred must be a float32"):
        abs_scores(p.double(), y, 1.0, 0.0, False, out)
    with pytest.raises(TypeError, match="y must be a float32"):
        abs_scores(p, y.cpu().numpy(), 1.0, 0.0, False, out)
    with pytest.raises(TypeError, match="out must be a float32"):
        abs_scores(p, y, 1.0, 0.0, False, out.double())
    with pytest.raises(ValueError, match="must be a non-empty vector"):
        abs_scores(p[:0], y[:0], 1.0, 0.0, False, out[:0])
    with pytest.raises(ValueError, match=r"y \(9,\) must have pred's shape \(10,\)"):
        abs_scores(p, y[:9], 1.0, 0.0, False, out)
    with pytest.raises(ValueError, match=r"out \(9,\) must have pred's shape"):
        abs_scores(p, y, 1.0, 0.0, False, out[:9])
    with pytest.raises(ValueError, match="on one GPU"):
        abs_scores(p, y.cpu(), 1.0, 0.0, False, out)
    with pytest.raises(ValueError, match="on one GPU"):
        abs_scores(p.cpu(), y.cpu(), 1.0, 0.0, False, out.cpu())
    with pytest.raises(ValueError, match="pred must be contiguous"):
        abs_scores(torch.zeros(2 * m, device=DEV)[::2], y, 1.0, 0.0, False, out)
    with pytest.raises(ValueError, match="out overlaps pred"):
        abs_scores(p, y, 1.0, 0.0, False, p)
    assert bool((out == 7.0).all())  # nothing was launched

    ids = np.arange(m) % 3
    with pytest.raises(ValueError, match=r"5 levels \(need 1 .. 4\)"):
        QuantilePlan(ids, 3, 5, DEV)
    with pytest.raises(ValueError, match=r"0 levels \(need 1 .. 4\)"):
        QuantilePlan(ids, 3, 0, DEV)
    with pytest.raises(ValueError, match=r"5000 groups x 4 levels = 20000 histograms \(need 1 .. 16384"):
        QuantilePlan(ids, 5000, 4, DEV)
    with pytest.raises(ValueError, match=r"group id 2 outside \[0, 2\)"):
        QuantilePlan(ids, 2, 1, DEV)
    plan = QuantilePlan(ids, 3, 2, DEV)
    assert plan.hist.shape == (3, 2, 256) and plan.state.shape == (3, 2, 2) and not bool(plan.hist.any())
    s = torch.ones(m, device=DEV)
    ranks = torch.zeros((3, 2), dtype=torch.int32, device=DEV)
    q = torch.full((3, 2), 7.0, device=DEV)
    with pytest.raises(TypeError, match="plan must be a QuantilePlan"):
        group_quantiles(s, plan.groups, ranks, q)
    with pytest.raises(TypeError, match="scores must be a torch.float32"):
        group_quantiles(s.double(), plan, ranks, q)
    with pytest.raises(TypeError, match="ranks must be a torch.int32"):
        group_quantiles(s, plan, ranks.long(), q)
    with pytest.raises(TypeError, match="out must be a torch.float32"):
        group_quantiles(s, plan, ranks, q.double())
    with pytest.raises(ValueError, match="scores is on cpu"):
        group_quantiles(s.cpu(), plan, ranks, q)
    with pytest.raises(ValueError, match="ranks is on cpu"):
        group_quantiles(s, plan, ranks.cpu(), q)
    with pytest.raises(ValueError, match=r"scores holds \(9,\) scores, the plan groups 10"):
        group_quantiles(s[:9], plan, ranks, q)
    with pytest.raises(ValueError, match=r"ranks must be contiguous \[3\]\[2\] \(groups x levels\), got \(3, 1\)"):
        group_quantiles(s, plan, ranks[:, :1].contiguous(), q)
    with pytest.raises(ValueError, match=r"ranks must be contiguous \[3\]\[2\]"):
        group_quantiles(s, plan, torch.zeros((2, 3), dtype=torch.int32, device=DEV), q)
    with pytest.raises(ValueError, match=r"out must be contiguous \[3\]\[2\]"):
        group_quantiles(s, plan, ranks, torch.full((3, 4), 7.0, device=DEV)[:, ::2])
    assert bool((q == 7.0).all()) and not bool(plan.hist.any())  # nothing was launched
    # the binding refuses the same on its own (a direct caller): still before any launch
    g = plan.groups
    with pytest.raises(RuntimeError, match=r"5 levels \(at most 4\)"):
        lib().group_quantiles(s, g.order, g.pieces, plan.piece_group, torch.zeros((3, 5), dtype=torch.int32, device=DEV),
                              plan.hist, plan.state, q)
    with pytest.raises(RuntimeError, match=r"hist must be int32 \[3\]\[2\]\[256\]"):
        lib().group_quantiles(s, g.order, g.pieces, plan.piece_group, ranks, plan.hist[:2], plan.state, q)
    with pytest.raises(RuntimeError, match=r"out must be a contiguous fp32 \[3\]\[2\]"):
        lib().group_quantiles(s, g.order, g.pieces, plan.piece_group, ranks, plan.hist, plan.state, q[:2])
    with pytest.raises(RuntimeError, match="out overlaps pred / y"):
        lib().abs_scores(p, y, 1.0, 0.0, False, y)
    assert bool((q == 7.0).all()) and bool((y == 1.0).all())


# ------------------------------------------------------------------ 3. the native job
@pytest.fixture(scope="module")
def fitted(tmp_path_factory):
    """An MLP (18 -> 256 -> 256 -> 1) fitted for a few hundred steps on the synthetic table (8 wells
    x 125 steps), and an LSTM with drawn weights on the same pipeline (the fixture of the other job
    tests)."""
    from wellflow.models.lstm import LSTMRegressor
    from wellflow.models.mlp import MLPRegressor

    d = tmp_path_factory.mktemp("interval_gpu")
    schema = parse_schema(NAMES, TYPES)
    table = load_table("synth", schema, synth_wells=8, synth_steps=125, seed=3)
    pipe = FeaturePipeline(schema, "flow", standardize_target=True).fit(table)
    assert pipe.n_features == 18
    torch.manual_seed(0)
    ref = MLPRegressor(18, (256, 256))
    X = torch.from_numpy(pipe.features(table))
    y = torch.from_numpy(np.asarray(pipe.target_values(table), np.float32)).reshape(-1)
    opt = torch.optim.Adam(ref.parameters(), lr=2e-3)
    threads = torch.get_num_threads()
    torch.set_num_threads(1)  # one order of additions: the fit does not depend on the machine's core count
    try:
        for _ in range(200):
            opt.zero_grad()
            ((ref(X).reshape(-1) - y) ** 2).mean().backward()
            opt.step()
    finally:
        torch.set_num_threads(threads)
    pm = str(d / "models" / "mlp.mdl")
    save_mdl(pm, "mlp", registry.keras_layers("mlp", ref), {"features": pipe.state()})
    pl = str(d / "models" / "lstm.mdl")
    save_mdl(pl, "lstm", registry.keras_layers("lstm", LSTMRegressor(18, 128)),
             {"features": pipe.state(), "job": {"seq_len": 8, "group_col": "well", "hidden": 128}})
    return dict(schema=schema, table=table, pipe=pipe, mlp=pm, lstm=pl, dir=d)


def host_rule(pred, table, alphas, by, relative, piece_rows=0):
    """The bands of the numpy rule over the ENGINE's own predictions, copied to the host."""
    from wellflow.interval import group_quantiles_host, make_bands, score_host, select_ranks
    from wellflow.whatif import scorer_for

    scorer = scorer_for(pred, table, "interval", piece_rows)
    with torch.no_grad():
        p = scorer.predict().cpu().numpy()
    y = np.asarray(table["flow"], np.float32)
    groups, ids = np.unique(np.asarray(table[by]).astype(str), return_inverse=True)
    if scorer.rows is not None:
        y, ids = y[scorer.rows], ids[scorer.rows]
    G, M = len(groups), len(p)
    counts = np.bincount(ids, minlength=G)
    s = score_host(p, y, scorer.y_scale, scorer.y_shift, relative)
    q_all = group_quantiles_host(s, np.zeros(M, np.int64), 1, select_ranks([M], alphas))[0]
    q_by = group_quantiles_host(s, ids, G, select_ranks(counts, alphas))
    return make_bands(by, relative, alphas, [str(g) for g in groups], counts, q_by, M, q_all, lambda s: None)


def _same_bands(got, want, tmp, tag):
    from wellflow.interval import write_bands

    assert [tuple(r.values()) for r in got["rows"]] == [tuple(r.values()) for r in want["rows"]], tag
    a, b = str(tmp / f"{tag}_device.csv"), str(tmp / f"{tag}_host.csv")
    write_bands(a, got)
    write_bands(b, want)
    assert open(a).read() == open(b).read() and len(open(a).read().splitlines()) == 1 + len(want["rows"])


def test_native_mlp_calibration_equals_the_numpy_rule(fitted, tmp_path):
    from wellflow.interval import ConformalBands
    from wellflow.predict import Predictor

    schema, table = fitted["schema"], fitted["table"]
    alphas = ("0.1", "0.05", "0.5")
    pred = Predictor.load(fitted["mlp"], schema, device="cuda", precision="bf16", batch=512)
    for relative in (False, True):
        job = ConformalBands(pred, alphas=alphas, by="well", relative=relative)
        bands = job.calibrate(table)
        assert bands["native"] and bands["scored"] == 1000 and pred.eng_batch == 512 and len(bands["rows"]) == 27
        assert all(r["source"] == "group" for r in bands["rows"] if r["group"])
        _same_bands(bands, host_rule(pred, table, list(alphas), "well", relative), tmp_path, f"whole{int(relative)}")
        # the assembled table in pieces of 512 rows
        pieced = ConformalBands(pred, alphas=alphas, by="well", relative=relative, piece_rows=512).calibrate(table)
        _same_bands(pieced, bands, tmp_path, f"pieces{int(relative)}")
    # a group too small for its own band, on the device path
    few = take(table, np.flatnonzero((np.asarray(table["well"]).astype(str) != "W007") | (np.arange(1000) % 125 < 5)))
    fb = ConformalBands(pred, alphas=alphas, by="well").calibrate(few)
    assert [(r["rows"], r["source"]) for r in fb["rows"] if r["group"] == "W007"] == [(5, "overall"), (5, "overall"), (5, "group")]
    _same_bands(fb, host_rule(pred, few, list(alphas), "well", False), tmp_path, "few")


def test_native_lstm_calibration_equals_the_numpy_rule(fitted, tmp_path):
    from wellflow.interval import ConformalBands
    from wellflow.predict import Predictor

    schema, table = fitted["schema"], fitted["table"]
    sub = take(table, np.arange(0, 1000, 5))  # 200 rows, 25 per well: 8 x 18 = 144 windows, three launches of 64
    pred = Predictor.load(fitted["lstm"], schema, device="cuda", precision="bf16", batch=64)
    alphas = ("0.1", "0.5")
    bands = ConformalBands(pred, alphas=alphas, by="well").calibrate(sub)
    assert bands["native"] and pred.eng_batch == 64 and bands["scored"] == 144
    assert [r["rows"] for r in bands["rows"][:9]] == [144] + [18] * 8
    _same_bands(bands, host_rule(pred, sub, list(alphas), "well", False), tmp_path, "lstm")
    assert pred.eng.persistent_error() == 0, pred.eng.persistent_stats()


# ------------------------------------------------------------------ 4. end to end
def test_train_calibrate_apply_on_the_gpu(tmp_path):
    from wellflow.interval import conformal_rank, read_bands, run_interval
    from wellflow.train.job import run_job

    sp = str(tmp_path) + "/"
    out = run_job("mlp", [NAMES, TYPES, "flow", sp, "--max-steps", "60", "--synth-wells", "4", "--synth-steps", "200",
                          "--verbose", "0"], **QUIET)
    assert out["native"]
    schema = parse_schema(NAMES, TYPES)
    table = load_table("synth", schema, synth_wells=4, synth_steps=200, seed=42)
    path = str(tmp_path / "data.csv")
    write_csv(table, path, columns=NAMES.split(","))
    args = [NAMES, TYPES, "flow", sp, path]
    lines = []
    cal = run_interval("mlp", args + ["--calibrate", "--alpha", "0.1,0.2", "--by", "well"], log=lambda s: lines.append(str(s)))
    assert cal["native"] and cal["scored"] == 800 and cal["out"] == sp + "interval/mlp.bands.csv"
    assert lines[0] == "Calibration rows scored: 800" and lines[1].startswith("Overall quantile 90: ") and len(lines) == 3
    bands = read_bands(cal["out"])
    assert [r["rank"] for r in bands["rows"][:2]] == [conformal_rank(800, "0.1"), conformal_rank(200, "0.1")]
    lines.clear()
    res = run_interval("mlp", args, log=lambda s: lines.append(str(s)))
    assert res["native"] and res["scored"] == 800 and res["out"] == sp + "interval/mlp.csv"
    with open(res["out"], newline="") as f:
        rows = list(csv.reader(f))
    assert rows[0] == NAMES.split(",") + ["prediction", "lower_90", "upper_90", "lower_80", "upper_80", "band"] and len(rows) == 801
    print("end to end:", lines)
    assert lines[:2] == ["Rows scored: 800", "Rows without prediction: 0"] and lines[2].startswith("Empirical coverage 90: ")
    # the calibration rows, re-scored: every group with its own band is covered at its level
    y = np.asarray(load_table(path, schema)["flow"], np.float64)  # what the job parsed
    wells = np.asarray([r[0] for r in rows[1:]])
    assert {r[15] for r in rows[1:]} == {"group"}
    for a, alpha in enumerate(("0.1", "0.2")):
        lo = np.asarray([float(r[11 + 2 * a]) for r in rows[1:]])
        hi = np.asarray([float(r[12 + 2 * a]) for r in rows[1:]])
        inside = (lo <= y) & (y <= hi)
        assert inside.mean() >= 1 - float(alpha) and res["coverage"][a] == inside.mean()
        for w in np.unique(wells):
            assert inside[wells == w].mean() >= 1 - float(alpha), (alpha, w)


# ------------------------------------------------------------------ 5. against the fp32 oracle
# Measured on an MI355X for this file's fixed seeds (profiles/r7/interval/README.md) and asserted at
# twice the recorded worst case: the bf16 engine's predictions differ from the fp32 oracle's, so each
# residual moves by about the bf16 error of the prediction and the order statistics move with them.
ORACLE_QUANTILE_REL = 2 * 0.0703013  # max |q_native - q_oracle| / q_oracle over the 27 quantiles (measured: 0.0703013,
#                                       median 0.0078)


def test_native_mlp_quantiles_against_the_fp32_oracle(fitted):
    from wellflow.interval import ConformalBands
    from wellflow.predict import Predictor

    schema, table = fitted["schema"], fitted["table"]
    alphas = ("0.1", "0.05", "0.5")
    pred = Predictor.load(fitted["mlp"], schema, device="cuda", precision="bf16", batch=512)
    bands = ConformalBands(pred, alphas=alphas, by="well").calibrate(table)
    cpu = Predictor.load(fitted["mlp"], schema, device="cpu", precision="fp32")
    ora = ConformalBands(cpu, alphas=alphas, by="well").calibrate(table)
    assert not ora["native"]
    qn = np.asarray([r["quantile"] for r in bands["rows"]])
    qo = np.asarray([r["quantile"] for r in ora["rows"]])
    rel = np.abs(qn - qo) / qo
    print("vs fp32 oracle: quantile relative difference: max %.6g median %.6g over %d quantiles" %
          (float(rel.max()), float(np.median(rel)), len(rel)))
    assert float(rel.max()) <= ORACLE_QUANTILE_REL
