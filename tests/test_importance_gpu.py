"""Permutation importance on the GPU: the assembly kernel's permuted source column bit for bit
(csrc/features.hip), the fp64 scoring-error reduction (csrc/score.hip) and the native pass loops of
wellflow/importance.py against the same engines fed from the host."""
import csv
import types

import numpy as np
import pytest
import torch

from wellflow.data.features import FeaturePipeline, take, window_starts
from wellflow.data.io import load_table, write_csv
from wellflow.data.schema import parse_schema
from wellflow.models import registry
from wellflow.utils.checkpoint import save_mdl

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0) if torch.cuda.is_available() else None

NAMES = "well,field,t,whp,choke,glr,temp,water_cut,dsp,flow"
TYPES = "string,string,int,float,float,float,float,float,float,float"
INPUTS = ["well", "field", "t", "whp", "choke", "glr", "temp", "water_cut", "dsp"]
QUIET = dict(log=lambda *a, **k: None)
EPS = 2.0 ** -52


# ------------------------------------------------------------------ 1. the permuted assembly
N_MAX = 4099
SIZES = [1, 63, 64, 65, 1000, N_MAX]
# (label counts per categorical column, continuous columns): F = sum(labels) + Q
COLUMN_SETS = {
    "q1": ((), 1),
    "c3_17_q7": ((3, 17), 7),        # F = 27, Fp = 32
    "c40_q9": ((40,), 9),            # F = 49, Fp = 56
    "c3_17_q0": ((3, 17), 0),        # F = 20, Fp = 24
    "c7_q1": ((7,), 1),              # F = 8: no padding
}
_REF = {}


def _reference(key):
    """(pipe, table) of a column set; the pipeline is fitted on rows without unseen labels."""
    if key in _REF:
        return _REF[key]
    labels, Q = COLUMN_SETS[key]
    rng = np.random.default_rng(len(key) * 1000 + Q)
    names = [f"c{i}" for i in range(len(labels))] + [f"x{i}" for i in range(Q)] + ["y"]
    kinds = ["string"] * len(labels) + ["float"] * Q + ["float"]
    schema = parse_schema(",".join(names), ",".join(kinds))
    table = {}
    for i, L in enumerate(labels):
        # label k drawn with weight ~ 1 / (k + 1), so the frequency order is not the label order;
        # 'unseen' never occurs in the rows the pipeline is fitted on
        p = 1.0 / (1.0 + np.arange(L + 1))
        p[-1] = 0.05 * p[:-1].sum()
        pool = np.asarray([f"l{k:02d}" for k in range(L)] + ["unseen"], dtype=object)
        table[f"c{i}"] = pool[rng.choice(L + 1, size=N_MAX, p=p / p.sum())]
    for i in range(Q):  # finite, 1e-3 <= |x| <= 1e4: no standardised value is denormal
        mag = 10.0 ** rng.uniform(-3.0, 4.0, size=N_MAX)
        table[f"x{i}"] = (mag * rng.choice([-1.0, 1.0], size=N_MAX)).astype(np.float32)
    table["y"] = rng.normal(size=N_MAX).astype(np.float32)
    seen = np.ones(N_MAX, bool)
    for i in range(len(labels)):
        seen &= table[f"c{i}"] != "unseen"
    fit_rows = np.flatnonzero(seen)[:2000]
    pipe = FeaturePipeline(schema, "y").fit(take(table, fit_rows))
    assert [len(ix.labels) for ix in pipe.indexers] == list(labels) and pipe.n_features == sum(labels) + Q
    _REF[key] = (pipe, table)
    return _REF[key]


def _perm_sources(C, Q):
    """First and last categorical column, first and last continuous column (source order)."""
    srcs = []
    for k in ([0, C - 1] if C else []) + ([C, C + Q - 1] if Q else []):
        if k not in srcs:
            srcs.append(k)
    return srcs


def _perms(n, seed):
    rng = np.random.default_rng(seed)
    return {"identity": np.arange(n), "reversal": np.arange(n)[::-1].copy(), "random": rng.permutation(n),
            "repeated": rng.integers(0, n, size=n)}


def _bits(t):
    t = t.cpu()
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("key", list(COLUMN_SETS))
def test_permuted_assembly_is_bit_exact(key, n):
    from wellflow.models.mlp import NativeMLP
    from wellflow.ops.native import ResidentColumns, assemble_features

    pipe, table = _reference(key)
    sub = take(table, np.arange(n))
    codes, cont = pipe.raw_columns(sub)
    off, size = pipe.block_spec()
    mean, std = pipe.scale()
    F = pipe.n_features
    Fp = (F + 7) // 8 * 8
    stub = types.SimpleNamespace(F=F, Fp=Fp)
    names = [ix.column for ix in pipe.indexers] + list(pipe.continuous)
    C, Q = codes.shape[0], cont.shape[0]
    res = ResidentColumns(codes, cont, off, size, mean, std, F, DEV)
    assert (res.C, res.Q, res.N) == (C, Q, n)
    plain = {dt: assemble_features(codes, cont, off, size, mean, std, F, dt, DEV) for dt in (torch.float32, torch.bfloat16)}
    for dt in plain:  # perm_src = -1 through the new call shape: the existing launch
        assert torch.equal(_bits(res.assemble(dt)), _bits(plain[dt]))
    for k in _perm_sources(C, Q):
        for what, perm in _perms(n, 17 * n + k).items():
            t2 = dict(sub)
            t2[names[k]] = np.asarray(sub[names[k]])[perm]
            want32 = torch.from_numpy(pipe.features(t2))                       # (a) the host pipeline
            codes2, cont2 = codes.copy(), cont.copy()
            if k < C:
                codes2[k] = codes[k][perm]
            else:
                cont2[k - C] = cont[k - C][perm]
            pd = torch.from_numpy(perm.astype(np.int32)).to(DEV)
            for dt, ld in ((torch.float32, F), (torch.bfloat16, Fp)):
                out = torch.full((n, ld), float("nan"), dtype=dt, device=DEV)  # unwritten padding would show
                got = res.assemble(dt, perm=pd, perm_col=k, out=out)
                torch.cuda.synchronize()
                assert got.data_ptr() == out.data_ptr()
                want = want32 if dt == torch.float32 else NativeMLP.to_input_format(stub, want32)
                assert torch.equal(_bits(out), _bits(want)), (key, n, k, what, dt)
                unperm = assemble_features(codes2, cont2, off, size, mean, std, F, dt, DEV)  # (b)
                assert torch.equal(_bits(out), _bits(unperm)), (key, n, k, what, dt)
                if what == "identity":
                    assert torch.equal(_bits(out), _bits(plain[dt]))


@pytest.mark.parametrize("key", ["c3_17_q7", "c40_q9"])
def test_permuted_assembly_of_a_piece(key):
    """Output rows [64, 200) of N = 1000 with a permutation that indexes all 1000 rows."""
    from wellflow.ops.native import ResidentColumns

    pipe, table = _reference(key)
    n, a, b = 1000, 64, 200
    codes, cont = pipe.raw_columns(take(table, np.arange(n)))
    res = ResidentColumns(codes, cont, *pipe.block_spec(), *pipe.scale(), pipe.n_features, DEV)
    perm = torch.from_numpy(np.random.default_rng(3).permutation(n).astype(np.int32)).to(DEV)
    assert int(perm[a:b].max()) >= b and int(perm[a:b].min()) < a  # the piece reads outside itself
    for k in _perm_sources(res.C, res.Q):
        for dt in (torch.float32, torch.bfloat16):
            whole = res.assemble(dt, perm=perm, perm_col=k)
            out = torch.full((b - a, whole.shape[1]), float("nan"), dtype=dt, device=DEV)
            res.assemble(dt, rows=(a, b), perm=perm[a:b], perm_col=k, out=out)
            assert torch.equal(_bits(out), _bits(whole[a:b])), (k, dt)
            assert torch.equal(_bits(res.assemble(dt, rows=(a, b))), _bits(res.assemble(dt)[a:b]))


def test_permuted_assembly_refusals_come_from_the_host():
    from wellflow.ops.native import ResidentColumns

    pipe, table = _reference("c3_17_q7")
    n = 130
    codes, cont = pipe.raw_columns(take(table, np.arange(n)))
    res = ResidentColumns(codes, cont, *pipe.block_spec(), *pipe.scale(), pipe.n_features, DEV)
    good = torch.arange(n, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match="for 130 rows"):
        res.assemble(torch.float32, perm=good[:129], perm_col=0)
    with pytest.raises(ValueError, match="for 66 rows"):
        res.assemble(torch.float32, rows=(64, 130), perm=good, perm_col=0)
    with pytest.raises(TypeError, match="int32"):
        res.assemble(torch.float32, perm=good.long(), perm_col=0)
    for bad in (9, 100):  # C + Q = 9 sources: 0 .. 8
        with pytest.raises(ValueError, match=r"perm_col \d+ outside \[0, 9\)"):
            res.assemble(torch.float32, perm=good, perm_col=bad)
    with pytest.raises(ValueError, match="go together"):
        res.assemble(torch.float32, perm=good)
    with pytest.raises(ValueError, match="go together"):
        res.assemble(torch.float32, perm_col=2)
    with pytest.raises(ValueError, match="must be a tensor on"):
        res.assemble(torch.float32, perm=good.cpu(), perm_col=0)
    with pytest.raises(ValueError, match="outside the table's 130 rows"):
        res.assemble(torch.float32, rows=(64, 131))


# ------------------------------------------------------------------ 2. err_sums
def _host_sums(pred, y, ys, sh):
    d = pred.astype(np.float64) * ys + sh - y.astype(np.float64)
    return np.asarray([np.sum(d * d), np.sum(np.abs(d))])


@pytest.mark.parametrize("m", [1, 63, 257, 70001])
def test_err_sums(m):
    from wellflow.ops.native import err_sums, err_sums_scratch

    rng = np.random.default_rng(m)
    pred = rng.normal(size=m).astype(np.float32)
    y = (rng.normal(size=m) * 40 + 100).astype(np.float32)
    ys, sh = 37.25 + 1.0 / 3.0, 101.0 / 7.0
    want = _host_sums(pred, y, ys, sh)
    pd, yd = torch.from_numpy(pred).to(DEV), torch.from_numpy(y).to(DEV)
    out = torch.full((3, 2), -7.0, dtype=torch.float64, device=DEV)
    scratch = err_sums_scratch(DEV)
    err_sums(pd, yd, ys, sh, out, 0, scratch)
    first = out.cpu().numpy().copy()
    assert (first[1:] == -7.0).all()  # the other slots are untouched
    rel = np.abs(first[0] - want) / want
    print(f"err_sums M={m}: rel err {rel}, bound {m * EPS}")
    assert (rel <= m * EPS).all(), (rel, m * EPS)
    err_sums(pd, yd, ys, sh, out, 2, scratch)  # a second launch, another slot: bitwise the same
    second = out.cpu().numpy()
    assert np.array_equal(second[2].view(np.int64), first[0].view(np.int64))
    assert np.array_equal(second[0].view(np.int64), first[0].view(np.int64)) and (second[1] == -7.0).all()
    assert int(scratch[-1:].view(torch.int64).item()) == 0  # the ticket is left at zero
    # one NaN prediction: NaN sums, reported not hidden
    bad = pd.clone()
    bad[m // 2] = float("nan")
    err_sums(bad, yd, ys, sh, out, 1, scratch)
    assert torch.isnan(out[1]).all().item()
    # ... and a launch after it still gives the right answer
    err_sums(pd, yd, 1.0, 0.0, out, 1, scratch)
    third = out.cpu().numpy()
    want1 = _host_sums(pred, y, 1.0, 0.0)
    assert (np.abs(third[1] - want1) / want1 <= m * EPS).all()
    assert np.array_equal(third[0].view(np.int64), first[0].view(np.int64))


def test_err_sums_refusals():
    from wellflow.ops.native import err_sums, err_sums_scratch

    p = torch.zeros(10, device=DEV)
    out = torch.zeros((2, 2), dtype=torch.float64, device=DEV)
    scratch = err_sums_scratch(DEV)
    with pytest.raises(ValueError, match="equal, non-empty"):
        err_sums(p, p[:9], 1.0, 0.0, out, 0, scratch)
    with pytest.raises(TypeError, match="float32"):
        err_sums(p.double(), p, 1.0, 0.0, out, 0, scratch)
    with pytest.raises(ValueError, match="slot 2"):
        err_sums(p, p, 1.0, 0.0, out, 2, scratch)
    with pytest.raises(RuntimeError, match="scratch"):
        err_sums(p, p, 1.0, 0.0, out, 0, scratch[:100])


# ------------------------------------------------------------------ 3. the native MLP passes
def _print_table(title, res):
    print(title, "baseline_mse", res["baseline_mse"])
    for d in res["importance"]:
        print("   %-10s importance %.9g  mean %.9g" % (d["column"], d["importance"], d["permuted_mse_mean"]))


def test_native_mlp_passes_equal_host_fed_engine(tmp_path):
    from wellflow.importance import PermutationImportance
    from wellflow.models.mlp import MLPRegressor
    from wellflow.predict import Predictor

    schema = parse_schema(NAMES, TYPES)
    table = load_table("synth", schema, synth_wells=8, synth_steps=125, seed=3)
    pipe = FeaturePipeline(schema, "flow", standardize_target=True).fit(table)
    assert pipe.n_features == 18  # 8 well columns + 3 field columns + 7 continuous
    torch.manual_seed(0)
    ref = MLPRegressor(18, (256, 256))
    with torch.no_grad():
        ref.linears()[0].weight[:, 8:11] = 0.0  # the first layer does not read the 'field' block
    p = str(tmp_path / "models" / "mlp.mdl")
    save_mdl(p, "mlp", registry.keras_layers("mlp", ref), {"features": pipe.state()})
    n, R = 1000, 2
    rng = np.random.default_rng(21)
    perms = torch.from_numpy(np.stack([np.stack([rng.permutation(n) for _ in range(R)]) for _ in INPUTS]))

    pred = Predictor.load(p, schema, device="cuda", precision="bf16", batch=512)
    res = PermutationImportance(pred, repeats=R).run(table, perms=perms)
    assert res["native"] and pred.eng_batch == 512 and res["scored"] == n and res["sums"].shape == (1 + 9 * R, 2)
    eng = pred.eng
    y = pipe.target_values(table, raw=True)

    def host_fed(tab):  # 1000 rows: a full chunk of 512 and a short one of 488
        Xh = eng.to_input_format(torch.from_numpy(pipe.features(tab))).to(DEV)
        out = torch.cat([eng.forward(Xh[a : a + 512]).clone() for a in (0, 512)]).cpu().numpy()
        return _host_sums(out, y, pipe.y_std, pipe.y_mean)

    want = [host_fed(table)]
    for i, c in enumerate(INPUTS):
        for r in range(R):
            t2 = dict(table)
            t2[c] = np.asarray(table[c])[perms[i, r].numpy()]
            want.append(host_fed(t2))
    want = np.asarray(want)
    rel = np.abs(res["sums"] - want) / want
    print("native MLP passes vs host-fed engine, max rel err", rel.max(), "bound", n * EPS)
    assert (rel <= n * EPS).all(), rel.max()
    by = {d["column"]: d for d in res["importance"]}
    assert by["field"]["importance"] == 0.0 and by["field"]["permuted_mse"] == [res["baseline_mse"]] * R

    # the assembled table in pieces of 512 rows (the permuted column is gathered from all 1000)
    pieced = PermutationImportance(pred, repeats=R, piece_rows=512).run(table, perms=perms)
    relp = np.abs(pieced["sums"] - want) / want
    assert (relp <= n * EPS).all(), relp.max()
    assert np.array_equal(pieced["sums"], res["sums"])  # the same launches on the same rows

    # the ranking against the fp32 oracle on the same permutations
    cpu = Predictor.load(p, schema, device="cpu", precision="fp32")
    ora = PermutationImportance(cpu, repeats=R).run(table, perms=perms)
    _print_table("native bf16:", res)
    _print_table("fp32 oracle:", ora)
    gap = abs(res["baseline_mse"] - ora["baseline_mse"])
    print("baseline gap", gap)
    oby = {d["column"]: d["importance"] for d in ora["importance"]}
    checked = 0
    for i, a in enumerate(INPUTS):
        for b in INPUTS[i + 1 :]:
            if abs(oby[a] - oby[b]) > gap:
                checked += 1
                assert (by[a]["importance"] > by[b]["importance"]) == (oby[a] > oby[b]), (a, b)
    assert checked > 0 and oby["field"] == 0.0


def test_native_mlp_draws_its_permutations_on_the_device(tmp_path):
    """No injected perms: torch.randperm on the device; the same seed gives the same sums."""
    from wellflow.importance import PermutationImportance
    from wellflow.models.mlp import MLPRegressor
    from wellflow.predict import Predictor

    schema = parse_schema(NAMES, TYPES)
    table = load_table("synth", schema, synth_wells=8, synth_steps=125, seed=3)
    pipe = FeaturePipeline(schema, "flow", standardize_target=True).fit(table)
    torch.manual_seed(0)
    p = str(tmp_path / "models" / "mlp.mdl")
    save_mdl(p, "mlp", registry.keras_layers("mlp", MLPRegressor(18, (256, 256))), {"features": pipe.state()})
    pred = Predictor.load(p, schema, device="cuda", precision="bf16", batch=512)
    a = PermutationImportance(pred, repeats=2, seed=5).run(table, columns=["whp", "well"])
    b = PermutationImportance(pred, repeats=2, seed=5).run(table, columns=["whp", "well"])
    c = PermutationImportance(pred, repeats=2, seed=6).run(table, columns=["whp", "well"])
    assert a["native"] and np.array_equal(a["sums"], b["sums"])
    assert np.array_equal(a["sums"][0], c["sums"][0]) and not np.array_equal(a["sums"][1:], c["sums"][1:])
    assert np.isfinite(a["sums"]).all() and (a["sums"][1:, 0] != a["sums"][0, 0]).all()


def test_wide_tables_take_the_host_path_with_the_native_engines(tmp_path, monkeypatch):
    """Above the device assembly's width limit the features are built on the host (announced once)
    and the native engines score them: the same sums as the device pass loop."""
    from wellflow.importance import PermutationImportance
    from wellflow.models.lstm import LSTMRegressor
    from wellflow.models.mlp import MLPRegressor
    from wellflow.predict import Predictor

    schema = parse_schema(NAMES, TYPES)
    table = load_table("synth", schema, synth_wells=8, synth_steps=125, seed=3)
    pipe = FeaturePipeline(schema, "flow", standardize_target=True).fit(table)
    torch.manual_seed(0)
    pm = str(tmp_path / "models" / "mlp.mdl")
    save_mdl(pm, "mlp", registry.keras_layers("mlp", MLPRegressor(18, (256, 256))), {"features": pipe.state()})
    pl = str(tmp_path / "models" / "lstm.mdl")
    save_mdl(pl, "lstm", registry.keras_layers("lstm", LSTMRegressor(18, 128)),
             {"features": pipe.state(), "job": {"seq_len": 8, "group_col": "well", "hidden": 128}})
    n, R, cols = 1000, 1, ["field", "choke"]
    rng = np.random.default_rng(4)
    perms = torch.from_numpy(np.stack([np.stack([rng.permutation(n) for _ in range(R)]) for _ in cols]))
    for path, batch, scored in ((pm, 512, n), (pl, 64, 8 * (125 - 7))):
        dev = PermutationImportance(Predictor.load(path, schema, device="cuda", precision="bf16", batch=batch),
                                    repeats=R).run(table, columns=cols, perms=perms)
        with monkeypatch.context() as m:
            m.setattr("wellflow.ops.native.ASSEMBLE_MAX_F", 8)
            host = PermutationImportance(Predictor.load(path, schema, device="cuda", precision="bf16", batch=batch),
                                         repeats=R).run(table, columns=cols, perms=perms)
        assert dev["native"] and host["native"] and dev["scored"] == host["scored"] == scored
        rel = np.abs(dev["sums"] - host["sums"]) / host["sums"]
        print("host-assembled vs device pass loop, max rel err", rel.max(), "bound", scored * EPS)
        assert (rel <= scored * EPS).all(), rel.max()


# ------------------------------------------------------------------ 4. the native LSTM passes
def test_native_lstm_passes_equal_host_gathered_windows(tmp_path):
    from wellflow.importance import PermutationImportance
    from wellflow.models.lstm import LSTMRegressor
    from wellflow.predict import Predictor

    T, H, Q = 8, 128, 13
    names = ["well"] + [f"x{i}" for i in range(Q)] + ["y"]
    schema = parse_schema(",".join(names), ",".join(["string"] + ["float"] * (Q + 1)))
    rng = np.random.default_rng(11)
    n = 150
    table = {"well": np.asarray([f"W{k}" for k in np.arange(n) % 3], dtype=object)}  # interleaved series
    for i in range(Q):
        table[f"x{i}"] = rng.normal(size=n).astype(np.float32) * 3 + 1
    table["y"] = rng.normal(size=n).astype(np.float32)
    pipe = FeaturePipeline(schema, "y").fit(table)  # target left raw: predictions are network outputs
    assert pipe.n_features == 16
    torch.manual_seed(1)
    ref = LSTMRegressor(16, H)
    p = str(tmp_path / "models" / "lstm.mdl")
    save_mdl(p, "lstm", registry.keras_layers("lstm", ref),
             {"features": pipe.state(), "job": {"seq_len": T, "group_col": "well", "hidden": H, "mlp_hidden": [256, 256]}})
    pred = Predictor.load(p, schema, device="cuda", precision="bf16", batch=64)
    cols, R = ["well", "x0", "x12"], 2
    perms = torch.from_numpy(np.stack([np.stack([rng.permutation(n) for _ in range(R)]) for _ in cols]))
    res = PermutationImportance(pred, repeats=R).run(table, columns=cols, perms=perms)
    eng = pred.eng
    assert res["native"] and pred.eng_batch == 64 and eng.H == H and eng.T == T
    assert res["scored"] == 129 and res["rows"] == n  # three chunks of 64: the last holds one window
    ids = np.unique(table["well"].astype(str), return_inverse=True)[1]
    order = np.argsort(ids, kind="stable")
    stable = take(table, order)
    starts = np.asarray(window_starts(n, T, ids[order]))
    y_last = pipe.target_values(stable, raw=True)[starts + T - 1]

    def host_fed(tab):
        X = pipe.features(tab)
        Xw = torch.from_numpy(X[starts[:, None] + np.arange(T)[None, :]]).to(DEV)
        out = torch.cat([eng.forward(Xw[a : a + 64]).clone() for a in range(0, 129, 64)]).cpu().numpy()
        return _host_sums(out, y_last, 1.0, 0.0)

    want = [host_fed(stable)]
    for i, c in enumerate(cols):
        for r in range(R):
            t2 = dict(stable)
            t2[c] = np.asarray(stable[c])[perms[i, r].numpy()]
            want.append(host_fed(t2))
    want = np.asarray(want)
    rel = np.abs(res["sums"] - want) / want
    print("native LSTM passes vs host-gathered windows, max rel err", rel.max(), "bound", 129 * EPS)
    assert (rel <= 129 * EPS).all(), rel.max()
    assert eng.persistent_error() == 0, eng.persistent_stats()


# ------------------------------------------------------------------ 5. end to end
def test_train_then_importance_job_on_the_gpu(tmp_path):
    from wellflow.importance import CSV_COLUMNS, run_importance
    from wellflow.train.job import run_job

    sp = str(tmp_path) + "/"
    out = run_job("mlp", [NAMES, TYPES, "flow", sp, "--max-steps", "20", "--synth-wells", "4", "--synth-steps", "200",
                          "--verbose", "0"], **QUIET)
    assert out["native"]
    schema = parse_schema(NAMES, TYPES)
    table = load_table("synth", schema, synth_wells=4, synth_steps=200, seed=42)
    path = str(tmp_path / "data.csv")
    write_csv(table, path, columns=NAMES.split(","))
    res = run_importance("mlp", [NAMES, TYPES, "flow", sp, path, "--repeats", "2"], **QUIET)
    assert res["native"] and res["scored"] == 800 and np.isfinite(res["baseline_mse"])
    with open(res["out"], newline="") as f:
        rows = list(csv.reader(f))
    assert tuple(rows[0]) == CSV_COLUMNS and sorted(r[0] for r in rows[1:]) == sorted(INPUTS)
    vals = np.asarray([[float(v) for v in r[2:]] for r in rows[1:]])
    assert np.isfinite(vals).all() and (vals[:, 0] == res["baseline_mse"]).all()
    assert list(vals[:, 3]) == sorted(vals[:, 3], reverse=True)
