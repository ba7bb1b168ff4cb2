"""Shapley attribution on the GPU: the assembly kernel's set launch bit for bit (csrc/features.hip),
the per-row fp64 accumulation (csrc/score.hip attr_step) against a numpy float64 replay, and the
native pass loops of wellflow/explain.py against the same engines fed from the host."""
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


# ------------------------------------------------------------------ 1. the set assembly
# the column sets, sizes and formats of tests/test_importance_gpu.py
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


def _sets(C, Q):
    """empty, each single column, all categorical, all continuous, every other column, all."""
    S = C + Q
    sets = {"empty": []}
    for s in range(S):
        sets[f"one{s}"] = [s]
    sets.update(cat=list(range(C)), cont=list(range(C, S)), alternate=list(range(0, S, 2)), all=list(range(S)))
    return sets


def _perms(n, seed):
    rng = np.random.default_rng(seed)
    return {"identity": np.arange(n), "random": rng.permutation(n), "repeated": rng.integers(0, n, size=n)}


def _bits(t):
    t = t.cpu()
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("key", list(COLUMN_SETS))
def test_set_assembly_is_bit_exact(key, n):
    from wellflow.models.mlp import NativeMLP
    from wellflow.ops.native import ResidentColumns, assemble_features, column_masks

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
    sets = _sets(C, Q)
    masks = column_masks(list(sets.values()), C + Q, DEV)  # one upload: a launch points at its row
    assert masks.dtype == torch.int32 and tuple(masks.shape) == (len(sets), 1)
    plain = {dt: res.assemble(dt) for dt in (torch.float32, torch.bfloat16)}
    for what, perm in _perms(n, 31 * n + C).items():
        pd = torch.from_numpy(perm.astype(np.int32)).to(DEV)
        for i, (sname, cols) in enumerate(sets.items()):
            t2 = dict(sub)
            codes2, cont2 = codes.copy(), cont.copy()
            for k in cols:
                t2[names[k]] = np.asarray(sub[names[k]])[perm]
                if k < C:
                    codes2[k] = codes[k][perm]
                else:
                    cont2[k - C] = cont[k - C][perm]
            want32 = torch.from_numpy(pipe.features(t2))                          # (a) the host pipeline
            for dt, ld in ((torch.float32, F), (torch.bfloat16, Fp)):
                out = torch.full((n, ld), float("nan"), dtype=dt, device=DEV)     # unwritten padding would show
                got = res.assemble(dt, perm=pd, col_set=masks[i], out=out)
                assert got.data_ptr() == out.data_ptr()
                want = want32 if dt == torch.float32 else NativeMLP.to_input_format(stub, want32)
                assert torch.equal(_bits(out), _bits(want)), (key, n, sname, what, dt)
                unperm = assemble_features(codes2, cont2, off, size, mean, std, F, dt, DEV)  # (b) the plain kernel
                assert torch.equal(_bits(out), _bits(unperm)), (key, n, sname, what, dt)
                if sname == "empty" or what == "identity":
                    assert torch.equal(_bits(out), _bits(plain[dt])), (key, n, sname, what, dt)
                if len(cols) == 1:  # the existing single-column launch
                    one = res.assemble(dt, perm=pd, perm_col=cols[0])
                    assert torch.equal(_bits(out), _bits(one)), (key, n, sname, what, dt)


@pytest.mark.parametrize("key", ["c3_17_q7", "c40_q9"])
def test_set_assembly_of_a_piece_and_clamped_indices(key):
    """Output rows [64, 200) of N = 1000 with a permutation that indexes all 1000 rows; indices
    outside the column are clamped into it, not read."""
    from wellflow.ops.native import ResidentColumns, assemble_features, column_masks

    pipe, table = _reference(key)
    n, a, b = 1000, 64, 200
    codes, cont = pipe.raw_columns(take(table, np.arange(n)))
    off, size = pipe.block_spec()
    mean, std = pipe.scale()
    res = ResidentColumns(codes, cont, off, size, mean, std, pipe.n_features, DEV)
    S = res.C + res.Q
    perm = torch.from_numpy(np.random.default_rng(3).permutation(n).astype(np.int32)).to(DEV)
    assert int(perm[a:b].max()) >= b and int(perm[a:b].min()) < a  # the piece reads outside itself
    sets = [list(range(S)), list(range(0, S, 2)), [0, S - 1]]
    masks = column_masks(sets, S, DEV)
    for i in range(len(sets)):
        for dt in (torch.float32, torch.bfloat16):
            whole = res.assemble(dt, perm=perm, col_set=masks[i])
            out = torch.full((b - a, whole.shape[1]), float("nan"), dtype=dt, device=DEV)
            res.assemble(dt, rows=(a, b), perm=perm[a:b], col_set=masks[i], out=out)
            assert torch.equal(_bits(out), _bits(whole[a:b])), (i, dt)
    # out-of-range indices: the values of the clamped host gather
    wild = np.random.default_rng(5).integers(-3 * n, 4 * n, size=n)
    wild[:4] = [-1, n, -2 ** 31, 2 ** 31 - 1]
    assert (wild < 0).sum() > 100 and (wild >= n).sum() > 100
    cl = np.clip(wild, 0, n - 1)
    wd = torch.from_numpy(wild.astype(np.int32)).to(DEV)
    for i, cols in enumerate(sets):
        codes2, cont2 = codes.copy(), cont.copy()
        for k in cols:
            if k < res.C:
                codes2[k] = codes[k][cl]
            else:
                cont2[k - res.C] = cont[k - res.C][cl]
        for dt in (torch.float32, torch.bfloat16):
            got = res.assemble(dt, perm=wd, col_set=masks[i])
            want = assemble_features(codes2, cont2, off, size, mean, std, pipe.n_features, dt, DEV)
            assert torch.equal(_bits(got), _bits(want)), (i, dt)
            got = res.assemble(dt, rows=(a, b), perm=wd[a:b], col_set=masks[i])
            assert torch.equal(_bits(got), _bits(want[a:b])), (i, dt)


def test_set_assembly_refusals_come_from_the_host():
    from wellflow.ops.native import ResidentColumns, column_masks, lib

    pipe, table = _reference("c3_17_q7")
    n = 130
    codes, cont = pipe.raw_columns(take(table, np.arange(n)))
    res = ResidentColumns(codes, cont, *pipe.block_spec(), *pipe.scale(), pipe.n_features, DEV)
    good = torch.arange(n, dtype=torch.int32, device=DEV)
    mask = column_masks([[0, 3]], 9, DEV)[0]
    one = torch.zeros(1, dtype=torch.float32, device=DEV)
    with pytest.raises(ValueError, match="not combined with a constant"):
        res.assemble(torch.float32, perm=good, col_set=mask, const_col=4, const_value=one)
    with pytest.raises(ValueError, match="ONE perm_col, not both"):
        res.assemble(torch.float32, perm=good, perm_col=2, col_set=mask)
    with pytest.raises(TypeError, match="col_set must be int32"):
        res.assemble(torch.float32, perm=good, col_set=mask.long())
    with pytest.raises(ValueError, match=r"words for 9 source columns \(need 1\)"):
        res.assemble(torch.float32, perm=good, col_set=torch.zeros(2, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError, match="col_set must be a tensor on"):
        res.assemble(torch.float32, perm=good, col_set=mask.cpu())
    with pytest.raises(ValueError, match="needs perm"):
        res.assemble(torch.float32, col_set=mask)
    with pytest.raises(ValueError, match="for 130 rows"):
        res.assemble(torch.float32, perm=good[:129], col_set=mask)
    with pytest.raises(TypeError, match="perm must be int32"):
        res.assemble(torch.float32, perm=good.long(), col_set=mask)
    with pytest.raises(ValueError, match=r"source column 9 outside \[0, 9\)"):
        column_masks([[9]], 9)
    # the binding refuses the same on its own (a direct caller): still before any launch
    out = torch.empty((n, 27), device=DEV)
    args = (res.codes, res.cont, res.off, res.size, res.mean, res.std, 0, n, 27, out)
    with pytest.raises(RuntimeError, match="not both"):
        lib().assemble_features(*args, 2, good, set_mask=mask)
    with pytest.raises(RuntimeError, match="not combined with a constant"):
        lib().assemble_features(*args, -1, good, 4, one, set_mask=mask)
    with pytest.raises(RuntimeError, match="needs perm"):
        lib().assemble_features(*args, -1, None, set_mask=mask)
    with pytest.raises(RuntimeError, match="set_mask holds 2 words"):
        lib().assemble_features(*args, -1, good, set_mask=torch.zeros(2, dtype=torch.int32, device=DEV))


# ------------------------------------------------------------------ 2. attr_step
@pytest.mark.parametrize("m", [1, 63, 257, 70001])
def test_attr_step_equals_numpy_replay(m):
    from wellflow.ops.native import attr_step

    rng = np.random.default_rng(m)
    ys, sh = 37.25 + 1.0 / 3.0, 101.0 / 7.0
    K = 3
    passes = [rng.normal(size=m).astype(np.float32) * 3 for _ in range(6)]  # a start and 5 steps
    rows = [K, 0, 1, 2, 0, 1]

    def device(ps):
        acc = torch.full((K + 2, m), 0.5, dtype=torch.float64, device=DEV)  # row K + 1 is never named
        sq = torch.full((K + 2, m), 0.25, dtype=torch.float64, device=DEV)
        prev = torch.full((m,), float("nan"), device=DEV)  # a start does not read it
        for i, (p, row) in enumerate(zip(ps, rows)):
            pd = torch.from_numpy(p).to(DEV)
            before = acc.clone()
            attr_step(pd, prev, ys, sh, acc, sq, row, i == 0)
            assert torch.equal(prev.view(torch.int32), pd.view(torch.int32))  # p_prev = p_cur, bit for bit
            others = [r for r in range(K + 2) if r != row]
            assert torch.equal(acc[others].view(torch.int64), before[others].view(torch.int64))  # rows not named
        return acc.cpu().numpy(), sq.cpu().numpy()

    def host(ps):
        acc, sq = np.full((K + 2, m), 0.5), np.full((K + 2, m), 0.25)
        prev = None
        for i, (p, row) in enumerate(zip(ps, rows)):
            pc = p.astype(np.float64)
            d = pc * ys + sh if i == 0 else (pc - prev) * ys
            acc[row] += d
            sq[row] += d * d
            prev = pc
        return acc, sq

    acc, sq = device(passes)
    want_acc, want_sq = host(passes)
    assert np.array_equal(acc.view(np.int64), want_acc.view(np.int64))
    assert np.array_equal(sq.view(np.int64), want_sq.view(np.int64))
    assert (acc[K + 1] == 0.5).all() and (sq[K + 1] == 0.25).all()
    acc2, sq2 = device(passes)  # two runs are bitwise equal
    assert np.array_equal(acc2.view(np.int64), acc.view(np.int64)) and np.array_equal(sq2.view(np.int64), sq.view(np.int64))
    # a NaN prediction reaches its own cell only (and the step after it, through p_prev)
    bad = [p.copy() for p in passes]
    bad[2][m // 2] = np.nan
    nacc, nsq = device(bad)
    cell = np.zeros((K + 2, m), bool)
    cell[[1, 2], m // 2] = True  # passes 2 and 3 accumulate into rows 1 and 2
    assert np.isnan(nacc[cell]).all() and np.isnan(nsq[cell]).all()
    assert np.array_equal(nacc[~cell].view(np.int64), acc[~cell].view(np.int64))
    assert np.array_equal(nsq[~cell].view(np.int64), sq[~cell].view(np.int64))


def test_attr_step_refusals():
    from wellflow.ops.native import attr_step

    p, q = torch.zeros(10, device=DEV), torch.zeros(10, device=DEV)
    acc = torch.zeros((3, 10), dtype=torch.float64, device=DEV)
    sq = torch.zeros((3, 10), dtype=torch.float64, device=DEV)
    with pytest.raises(TypeError, match="p_cur must be a float32"):
        attr_step(p.double(), q, 1.0, 0.0, acc, sq, 0)
    with pytest.raises(ValueError, match="equal, non-empty"):
        attr_step(p, q[:9], 1.0, 0.0, acc, sq, 0)
    with pytest.raises(TypeError, match="acc must be a float64"):
        attr_step(p, q, 1.0, 0.0, acc.float(), sq, 0)
    with pytest.raises(ValueError, match=r"sq must be contiguous float64 \[K \+ 1\]\[10\]"):
        attr_step(p, q, 1.0, 0.0, acc, sq[:, :9], 0)
    with pytest.raises(ValueError, match="differ"):
        attr_step(p, q, 1.0, 0.0, acc, sq[:2], 0)
    with pytest.raises(ValueError, match="on one GPU"):
        attr_step(p, q.cpu(), 1.0, 0.0, acc, sq, 0)
    for row in (-1, 3):
        with pytest.raises(ValueError, match=r"row -?\d outside \[0, 3\)"):
            attr_step(p, q, 1.0, 0.0, acc, sq, row)
    with pytest.raises(RuntimeError, match="overlap"):
        attr_step(p, p, 1.0, 0.0, acc, sq, 0)
    assert (acc == 0).all().item() and (sq == 0).all().item()  # nothing was launched


# ------------------------------------------------------------------ 3. the native MLP job
def replay(score, picked, orders, perms, y_scale, y_shift):
    """The rule, written out on its own: ``score(columns, perm)`` -> fp32 outputs of the table with
    those columns read through perm. Returns the float64 tables and what is derived from them."""
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
    return {"acc": acc, "sq": sq, "phi": mean[:K], "base": mean[K],
            "std": np.sqrt(np.maximum(0.0, sq / R - mean * mean))[:K],
            "prediction": p_full.astype(np.float64) * y_scale + y_shift}


def _same(res, want, names=("acc", "sq", "phi", "base", "std", "prediction")):
    for name in names:
        assert res[name].shape == want[name].shape, name
        assert np.array_equal(res[name].view(np.int64), want[name].view(np.int64)), name


def _local_accuracy(res):
    K = len(res["columns"])
    gap = np.abs(res["base"] + res["phi"].sum(axis=0) - res["prediction"])
    scale = np.maximum(np.maximum(np.abs(res["base"]), np.abs(res["prediction"])), np.abs(res["phi"]).sum(axis=0))
    bound = 4 * (K + 1) * EPS * scale
    print("local accuracy: max gap / bound", float((gap / np.maximum(bound, 1e-300)).max()))
    assert (gap <= bound).all(), float((gap / bound).max())


def _draws(n, R, K, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.permutation(K) for _ in range(R)]), np.stack([rng.permutation(n) for _ in range(R)])


def test_native_mlp_job_equals_host_fed_engine(tmp_path):
    from wellflow.explain import ShapleyAttribution
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
    orders, perms = _draws(n, R, 9, 21)

    pred = Predictor.load(p, schema, device="cuda", precision="bf16", batch=512)
    res = ShapleyAttribution(pred, repeats=R).run(table, orders=orders, perms=perms)
    assert res["native"] and pred.eng_batch == 512 and res["scored"] == n and res["columns"] == INPUTS
    eng = pred.eng

    def host_fed(cols, perm):  # 1000 rows: a full chunk of 512 and a short one of 488
        t2 = dict(table)
        for c in cols:
            t2[c] = np.asarray(table[c])[perm]
        Xh = eng.to_input_format(torch.from_numpy(pipe.features(t2))).to(DEV)
        return torch.cat([eng.forward(Xh[a : a + 512]).clone() for a in (0, 512)]).cpu().numpy()

    want = replay(host_fed, INPUTS, orders, perms, float(pipe.y_std), float(pipe.y_mean))
    _same(res, want)
    k = INPUTS.index("field")
    assert (res["phi"][k] == 0.0).all() and (res["std"][k] == 0.0).all()
    _local_accuracy(res)

    # the assembled table in pieces of 512 rows (the permuted columns are gathered from all 1000)
    pieced = ShapleyAttribution(pred, repeats=R, piece_rows=512).run(table, orders=orders, perms=perms)
    _same(pieced, res)

    # the ranking against the fp32 oracle on the same draws
    cpu = Predictor.load(p, schema, device="cpu", precision="fp32")
    ora = ShapleyAttribution(cpu, repeats=R).run(table, orders=orders, perms=perms)
    gap = float(np.mean(np.abs(res["prediction"] - ora["prediction"])))
    for title, r in (("native bf16:", res), ("fp32 oracle:", ora)):
        print(title, "  ".join("%s %.6g" % (c, v) for c, v in zip(r["columns"], r["mean_abs"])))
    print("mean |prediction_native - prediction_oracle|", gap)
    nat, orc = res["mean_abs"], ora["mean_abs"]
    checked = 0
    for i in range(9):
        for j in range(i + 1, 9):
            if abs(orc[i] - orc[j]) > 2 * gap:
                checked += 1
                assert (nat[i] > nat[j]) == (orc[i] > orc[j]), (INPUTS[i], INPUTS[j])
    print("pairs that qualify:", checked, "of 36")
    assert checked >= 18 and orc[k] == 0.0

    # no injected draws: torch.randperm on the device; the seed decides them
    a, b, c = (ShapleyAttribution(pred, repeats=R, seed=s).run(table, columns=["whp", "well"]) for s in (5, 5, 6))
    assert a["native"] and a["columns"] == ["well", "whp"]
    _same(a, b)
    assert np.array_equal(a["prediction"], c["prediction"]) and not np.array_equal(a["acc"], c["acc"])
    assert np.isfinite(a["acc"]).all() and np.abs(a["phi"]).max() > 0
    _local_accuracy(a)


# ------------------------------------------------------------------ 4. the wide-table route
def test_wide_tables_take_the_host_path_with_the_native_engines(tmp_path, monkeypatch):
    """Above the device assembly's width limit the features are built on the host (announced once)
    and the native engines score them: the same tables as the device pass loop, bit for bit."""
    from wellflow.explain import ShapleyAttribution
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
    n, R, cols = 1000, 2, ["field", "choke", "whp"]
    orders, perms = _draws(n, R, 3, 4)
    for path, batch, scored in ((pm, 512, n), (pl, 64, 8 * (125 - 7))):
        dev = ShapleyAttribution(Predictor.load(path, schema, device="cuda", precision="bf16", batch=batch),
                                 repeats=R).run(table, columns=cols, orders=orders, perms=perms)
        with monkeypatch.context() as m:
            m.setattr("wellflow.ops.native.ASSEMBLE_MAX_F", 8)
            host = ShapleyAttribution(Predictor.load(path, schema, device="cuda", precision="bf16", batch=batch),
                                      repeats=R).run(table, columns=cols, orders=orders, perms=perms)
        assert dev["native"] and host["native"] and dev["scored"] == host["scored"] == scored
        assert np.abs(dev["phi"]).max() > 0
        _same(host, dev)


# ------------------------------------------------------------------ 5. the native LSTM
def test_native_lstm_job_equals_host_gathered_windows(tmp_path):
    from wellflow.explain import ShapleyAttribution
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
    orders, perms = _draws(n, R, 3, 13)
    res = ShapleyAttribution(pred, repeats=R).run(table, columns=cols, orders=orders, perms=perms)
    eng = pred.eng
    assert res["native"] and pred.eng_batch == 64 and eng.H == H and eng.T == T
    assert res["scored"] == 129 and res["n"] == n  # three chunks of 64: the last holds one window
    ids = np.unique(table["well"].astype(str), return_inverse=True)[1]
    order = np.argsort(ids, kind="stable")
    stable = take(table, order)
    starts = np.asarray(window_starts(n, T, ids[order]))
    assert np.array_equal(res["rows"], order[starts + T - 1])

    def host_fed(picked, perm):
        t2 = dict(stable)
        for c in picked:
            t2[c] = np.asarray(stable[c])[perm]
        X = pipe.features(t2)
        Xw = torch.from_numpy(X[starts[:, None] + np.arange(T)[None, :]]).to(DEV)
        return torch.cat([eng.forward(Xw[a : a + 64]).clone() for a in range(0, 129, 64)]).cpu().numpy()

    _same(res, replay(host_fed, cols, orders, perms, 1.0, 0.0))
    assert np.abs(res["phi"]).max() > 0
    _local_accuracy(res)
    # the default draws: orders, then the cyclic shifts, from the host generator
    auto = ShapleyAttribution(pred, repeats=R, seed=6).run(table, columns=cols)
    g = np.random.default_rng(6)
    o2 = np.stack([g.permutation(3) for _ in range(R)])
    shifts = g.integers(1, n, size=R)
    assert np.array_equal(auto["orders"], o2)
    _same(auto, replay(host_fed, cols, o2, np.stack([(np.arange(n) + s) % n for s in shifts]), 1.0, 0.0))
    assert eng.persistent_error() == 0, eng.persistent_stats()


# ------------------------------------------------------------------ 6. end to end
def test_train_then_explain_job_on_the_gpu(tmp_path):
    from wellflow.explain import run_explain
    from wellflow.train.job import run_job

    sp = str(tmp_path) + "/"
    out = run_job("mlp", [NAMES, TYPES, "flow", sp, "--max-steps", "20", "--synth-wells", "4", "--synth-steps", "200",
                          "--verbose", "0"], **QUIET)
    assert out["native"]
    schema = parse_schema(NAMES, TYPES)
    table = load_table("synth", schema, synth_wells=4, synth_steps=200, seed=42)
    path = str(tmp_path / "data.csv")
    write_csv(table, path, columns=NAMES.split(","))
    res = run_explain("mlp", [NAMES, TYPES, "flow", sp, path, "--repeats", "2", "--std"], **QUIET)
    assert res["native"] and res["scored"] == 800 and res["mse"] is not None and np.isfinite(res["mse"])
    with open(res["out"], newline="") as f:
        rows = list(csv.reader(f))
    assert rows[0] == NAMES.split(",") + ["prediction", "base"] + ["phi_" + c for c in INPUTS] + ["std_" + c for c in INPUTS]
    assert len(rows) == 801
    vals = np.asarray([[float(v) for v in r[10:]] for r in rows[1:]])
    assert np.isfinite(vals).all() and (vals[:, 11:] >= 0).all() and np.abs(vals[:, 2:11]).max() > 0
    gap = np.abs(vals[:, 1] + vals[:, 2:11].sum(axis=1) - vals[:, 0])
    scale = np.maximum(np.maximum(np.abs(vals[:, 0]), np.abs(vals[:, 1])), np.abs(vals[:, 2:11]).sum(axis=1))
    print("CSV local accuracy: max relative gap", float((gap / scale).max()))
    assert (gap <= 1e-9 * scale).all()
