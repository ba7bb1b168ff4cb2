"""Response curves on the GPU: the assembly kernel's constant source column bit for bit
(csrc/features.hip), the grouped fp64 prediction sums (csrc/score.hip group_sums) and the native pass
loops of wellflow/response.py against the same engines fed from the host."""
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
QUIET = dict(log=lambda *a, **k: None)
EPS = 2.0 ** -52


# ------------------------------------------------------------------ 1. the constant assembly
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


def _sources(C, Q):
    """First and last categorical column, first and last continuous column (source order)."""
    srcs = []
    for k in ([0, C - 1] if C else []) + ([C, C + Q - 1] if Q else []):
        if k not in srcs:
            srcs.append(k)
    return srcs


def _bits(t):
    t = t.cpu()
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


def _constants(pipe, k, C):
    """[(host value, one-element device tensor)] of source column k: the codes 0, L - 1 and L (the
    unknown index, label 'unseen') / the raw values 0, the column's fitted mean, 1e4, -3.5e-3."""
    if k < C:
        ix = pipe.indexers[k]
        L = len(ix.labels)
        codes = list(dict.fromkeys([0, L - 1, L]))
        grid = torch.tensor(codes, dtype=torch.int32, device=DEV)  # a grid uploaded once: pass g reads element g
        return [((ix.labels + ["unseen"])[c], c, grid[g : g + 1]) for g, c in enumerate(codes)]
    vals = np.asarray([0.0, pipe.scale()[0][k - C], 1e4, -3.5e-3], np.float32)
    grid = torch.from_numpy(vals).to(DEV)
    return [(v, v, grid[g : g + 1]) for g, v in enumerate(vals)]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("key", list(COLUMN_SETS))
def test_constant_assembly_is_bit_exact(key, n):
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
    fmt = lambda X32, dt: X32 if dt == torch.float32 else NativeMLP.to_input_format(stub, X32)  # noqa: E731
    # plain and permuted assembly through the new call shape: what they gave before (the host pipeline's bits)
    perm = np.random.default_rng(n).permutation(n)
    pd = torch.from_numpy(perm.astype(np.int32)).to(DEV)
    plain32 = torch.from_numpy(pipe.features(sub))
    for dt in (torch.float32, torch.bfloat16):
        assert torch.equal(_bits(res.assemble(dt, const_col=-1, const_value=None)), _bits(fmt(plain32, dt)))
        assert torch.equal(_bits(assemble_features(codes, cont, off, size, mean, std, F, dt, DEV)), _bits(fmt(plain32, dt)))
        k = _sources(C, Q)[-1]
        t2 = dict(sub)
        t2[names[k]] = np.asarray(sub[names[k]])[perm]
        got = res.assemble(dt, perm=pd, perm_col=k, const_col=-1, const_value=None)
        assert torch.equal(_bits(got), _bits(fmt(torch.from_numpy(pipe.features(t2)), dt)))
    for k in _sources(C, Q):
        for host, raw, dev in _constants(pipe, k, C):
            t2 = dict(sub)
            t2[names[k]] = np.full(n, host, object) if k < C else np.full(n, host, np.float32)
            want32 = torch.from_numpy(pipe.features(t2))                        # (a) the host pipeline
            codes2, cont2 = codes.copy(), cont.copy()
            if k < C:
                codes2[k] = raw
            else:
                cont2[k - C] = raw
            for dt, ld in ((torch.float32, F), (torch.bfloat16, Fp)):
                out = torch.full((n, ld), float("nan"), dtype=dt, device=DEV)   # unwritten padding would show
                got = res.assemble(dt, const_col=k, const_value=dev, out=out)
                torch.cuda.synchronize()
                assert got.data_ptr() == out.data_ptr()
                assert torch.equal(_bits(out), _bits(fmt(want32, dt))), (key, n, k, host, dt)
                over = assemble_features(codes2, cont2, off, size, mean, std, F, dt, DEV)  # (b)
                assert torch.equal(_bits(out), _bits(over)), (key, n, k, host, dt)
            if k < C and raw == len(pipe.indexers[k].labels):  # the unknown index: the all-zero block
                assert not want32[:, int(off[k]) : int(off[k]) + int(size[k])].any()


@pytest.mark.parametrize("key", ["c3_17_q7", "c40_q9"])
def test_constant_assembly_of_a_piece(key):
    """Output rows [64, 200) of N = 1000 equal the same rows of the whole."""
    from wellflow.ops.native import ResidentColumns

    pipe, table = _reference(key)
    n, a, b = 1000, 64, 200
    codes, cont = pipe.raw_columns(take(table, np.arange(n)))
    res = ResidentColumns(codes, cont, *pipe.block_spec(), *pipe.scale(), pipe.n_features, DEV)
    for k in _sources(res.C, res.Q):
        for _, _, dev in _constants(pipe, k, res.C):
            for dt in (torch.float32, torch.bfloat16):
                whole = res.assemble(dt, const_col=k, const_value=dev)
                out = torch.full((b - a, whole.shape[1]), float("nan"), dtype=dt, device=DEV)
                res.assemble(dt, rows=(a, b), const_col=k, const_value=dev, out=out)
                assert torch.equal(_bits(out), _bits(whole[a:b])), (k, dt)


def test_constant_assembly_refusals_come_from_the_host():
    from wellflow.ops.native import ResidentColumns

    pipe, table = _reference("c3_17_q7")
    n = 130
    codes, cont = pipe.raw_columns(take(table, np.arange(n)))
    res = ResidentColumns(codes, cont, *pipe.block_spec(), *pipe.scale(), pipe.n_features, DEV)
    code = torch.zeros(1, dtype=torch.int32, device=DEV)
    val = torch.zeros(1, dtype=torch.float32, device=DEV)
    good = torch.arange(n, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match="const_col and const_value go together"):
        res.assemble(torch.float32, const_value=code)
    with pytest.raises(ValueError, match="const_col and const_value go together"):
        res.assemble(torch.float32, const_col=1)
    with pytest.raises(ValueError, match="permuted or constant, not both"):
        res.assemble(torch.float32, perm=good, perm_col=0, const_col=1, const_value=code)
    for bad in (9, 100):  # C + Q = 9 sources: 0 .. 8
        with pytest.raises(ValueError, match=r"const_col \d+ outside \[0, 9\)"):
            res.assemble(torch.float32, const_col=bad, const_value=val)
    with pytest.raises(ValueError, match="must be a tensor on"):
        res.assemble(torch.float32, const_col=0, const_value=code.cpu())
    with pytest.raises(ValueError, match="must be a tensor on"):
        res.assemble(torch.float32, const_col=0, const_value=0)
    with pytest.raises(ValueError, match="one contiguous element"):
        res.assemble(torch.float32, const_col=0, const_value=torch.zeros(2, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError, match="one contiguous element"):
        res.assemble(torch.float32, const_col=2, const_value=torch.zeros(0, dtype=torch.float32, device=DEV))
    with pytest.raises(TypeError, match="int32 for a categorical"):
        res.assemble(torch.float32, const_col=1, const_value=val)
    with pytest.raises(TypeError, match="float32 for a continuous"):
        res.assemble(torch.float32, const_col=2, const_value=code)
    with pytest.raises(TypeError, match="float32 for a continuous"):
        res.assemble(torch.float32, const_col=8, const_value=val.double())
    # the existing refusals read as they did
    with pytest.raises(ValueError, match="perm and perm_col go together"):
        res.assemble(torch.float32, perm=good)
    with pytest.raises(ValueError, match="outside the table's 130 rows"):
        res.assemble(torch.float32, rows=(64, 131), const_col=0, const_value=code)


# ------------------------------------------------------------------ 2. group_sums
def _host_groups(pred, ids, G, ys, sh):
    v = pred.astype(np.float64) * ys + sh
    return np.stack([np.bincount(ids, minlength=G).astype(np.float64), np.bincount(ids, weights=v, minlength=G),
                     np.bincount(ids, weights=v * v, minlength=G)], axis=1), \
        np.bincount(ids, weights=np.abs(v), minlength=G)


def _check_groups(got, want, sabs, what):
    """n_g exact; |sum v - want| <= n_g 2^-52 sum|v|, |sum v^2 - want| <= n_g 2^-52 sum v^2 (the
    first-order bound between two fp64 summations in different orders); empty groups exact zeros."""
    assert np.array_equal(got[:, 0], want[:, 0]), what
    n = want[:, 0]
    e1, b1 = np.abs(got[:, 1] - want[:, 1]), n * EPS * sabs
    e2, b2 = np.abs(got[:, 2] - want[:, 2]), n * EPS * want[:, 2]
    i1, i2 = int(np.argmax(e1 - b1)), int(np.argmax(e2 - b2))
    print(f"{what}: sum v err {e1[i1]:.3g} (bound {b1[i1]:.3g}), sum v^2 err {e2[i2]:.3g} (bound {b2[i2]:.3g})")
    assert (e1 <= b1).all() and (e2 <= b2).all(), what
    assert (got[n == 0] == 0.0).all() and not np.signbit(got[n == 0]).any(), what


YS, SH = 37.25 + 1.0 / 3.0, 101.0 / 7.0  # not exactly representable


@pytest.mark.parametrize("layout", ["random", "sorted"])
@pytest.mark.parametrize("G", [1, 3, 1000])
@pytest.mark.parametrize("m", [1, 63, 257, 70001])
def test_group_sums(m, G, layout):
    from wellflow.ops.native import GroupPlan, group_sums

    rng = np.random.default_rng(m * 7 + G)
    pred = rng.normal(size=m).astype(np.float32)
    ids = rng.integers(0, G, size=m)
    if layout == "sorted":
        ids = np.sort(ids)
    want, sabs = _host_groups(pred, ids, G, YS, SH)
    plan = GroupPlan(ids, G, DEV)
    assert plan.M == m and plan.G == G and np.array_equal(plan.counts, want[:, 0])
    if layout == "sorted":
        assert torch.equal(plan.order.cpu(), torch.arange(m, dtype=torch.int32))  # the identity: a coalesced read
    pd = torch.from_numpy(pred).to(DEV)
    out = torch.full((3, G, 3), -7.0, dtype=torch.float64, device=DEV)
    group_sums(pd, plan, YS, SH, out, 0)
    first = out.cpu().numpy().copy()
    assert (first[1:] == -7.0).all()  # the other slots are untouched
    _check_groups(first[0], want, sabs, f"group_sums M={m} G={G} {layout}")
    group_sums(pd, plan, YS, SH, out, 2)  # a second launch, another slot: bitwise the same
    second = out.cpu().numpy()
    assert np.array_equal(second[2].view(np.int64), first[0].view(np.int64))
    assert np.array_equal(second[0].view(np.int64), first[0].view(np.int64)) and (second[1] == -7.0).all()
    # one NaN prediction: exactly its group is NaN
    bad = pd.clone()
    bad[m // 2] = float("nan")
    group_sums(bad, plan, YS, SH, out, 1)
    third = out.cpu().numpy()
    g = int(ids[m // 2])
    assert np.isnan(third[1, g, 1:]).all() and third[1, g, 0] == want[g, 0]
    others = np.arange(G) != g
    assert np.array_equal(third[1, others].view(np.int64), first[0, others].view(np.int64))
    # ... and a launch after it gives the right answer
    group_sums(pd, plan, 1.0, 0.0, out, 1)
    want1, sabs1 = _host_groups(pred, ids, G, 1.0, 0.0)
    _check_groups(out.cpu().numpy()[1], want1, sabs1, "after the NaN launch")


def test_group_sums_at_the_piece_boundary():
    """Three groups of P - 1, P and P + 1 predictions (P: positions per piece), interleaved."""
    from wellflow.ops.native import GROUP_PIECE as P, GroupPlan, group_sums

    rng = np.random.default_rng(5)
    ids = rng.permutation(np.repeat([0, 1, 2], [P - 1, P, P + 1]))
    pred = rng.normal(size=len(ids)).astype(np.float32)
    plan = GroupPlan(ids, 3, DEV)
    assert plan.group_pieces.tolist() == [0, 1, 2, 4] and plan.piece_group.tolist() == [0, 1, 2, 2]
    assert plan.pieces.tolist() == [[0, P - 1, 2 * P - 1, 3 * P - 1], [P - 1, P, P, 1]]
    out = torch.zeros((1, 3, 3), dtype=torch.float64, device=DEV)
    group_sums(torch.from_numpy(pred).to(DEV), plan, YS, SH, out, 0)
    want, sabs = _host_groups(pred, ids, 3, YS, SH)
    _check_groups(out.cpu().numpy()[0], want, sabs, "piece boundary")


def test_group_sums_refusals():
    from wellflow.ops.native import GROUP_SUMS_MAX_GROUPS, GroupPlan, group_sums

    ids = np.arange(10) % 3
    plan = GroupPlan(ids, 3, DEV)
    p = torch.zeros(10, device=DEV)
    out = torch.zeros((2, 3, 3), dtype=torch.float64, device=DEV)
    with pytest.raises(ValueError, match=r"group id 3 outside \[0, 3\)"):
        GroupPlan(np.asarray([0, 3, 1]), 3, DEV)
    with pytest.raises(ValueError, match=r"group id -1 outside \[0, 3\)"):
        GroupPlan(np.asarray([0, -1, 1]), 3, DEV)
    with pytest.raises(TypeError, match="integers"):
        GroupPlan(np.asarray([0.0, 1.0]), 3, DEV)
    with pytest.raises(ValueError, match=f"{GROUP_SUMS_MAX_GROUPS + 1} groups"):
        GroupPlan(ids, GROUP_SUMS_MAX_GROUPS + 1, DEV)
    with pytest.raises(TypeError, match="pred must be a float32"):
        group_sums(p.double(), plan, 1.0, 0.0, out, 0)
    with pytest.raises(TypeError, match="out must be a float64"):
        group_sums(p, plan, 1.0, 0.0, out.float(), 0)
    with pytest.raises(ValueError, match="the plan groups 10"):
        group_sums(p[:9], plan, 1.0, 0.0, out, 0)
    with pytest.raises(ValueError, match="slot 2"):
        group_sums(p, plan, 1.0, 0.0, out, 2)
    with pytest.raises(ValueError, match=r"\[S\]\[3\]\[3\]"):
        group_sums(p, plan, 1.0, 0.0, out[:, :2].contiguous(), 0)
    with pytest.raises(ValueError, match="pred is on cpu"):
        group_sums(p.cpu(), plan, 1.0, 0.0, out, 0)
    # the binding's own checks, behind the Python ones
    from wellflow.ops.native import lib

    with pytest.raises(RuntimeError, match="scratch"):
        lib().group_sums(p, plan.order, plan.pieces, plan.group_pieces, 1.0, 0.0, out, 0, plan.scratch[:3])
    with pytest.raises(RuntimeError, match="orders 10 predictions"):
        lib().group_sums(p[:9], plan.order, plan.pieces, plan.group_pieces, 1.0, 0.0, out, 0, plan.scratch)
    torch.cuda.synchronize()


# ------------------------------------------------------------------ 3. the native MLP passes
def _mlp_setup(tmp_path, blind=True):
    from wellflow.models.mlp import MLPRegressor

    schema = parse_schema(NAMES, TYPES)
    table = load_table("synth", schema, synth_wells=8, synth_steps=125, seed=3)
    pipe = FeaturePipeline(schema, "flow", standardize_target=True).fit(table)
    assert pipe.n_features == 18  # 8 well columns + 3 field columns + 7 continuous
    torch.manual_seed(0)
    ref = MLPRegressor(18, (256, 256))
    if blind:
        with torch.no_grad():
            ref.linears()[0].weight[:, 8:11] = 0.0  # the first layer does not read the 'field' block
    p = str(tmp_path / "models" / "mlp.mdl")
    save_mdl(p, "mlp", registry.keras_layers("mlp", ref), {"features": pipe.state()})
    return schema, table, pipe, p


def _replaced(table, col, value):
    t = dict(table)
    n = len(table[col])
    t[col] = np.full(n, value, object) if isinstance(value, str) else np.full(n, value, np.float32)
    return t


def _check_slots(got, want, what):
    for s in range(len(want)):
        _check_groups(got[s], want[s][0], want[s][1], f"{what} slot {s}")


def test_native_mlp_passes_equal_host_fed_engine(tmp_path):
    from wellflow.predict import Predictor
    from wellflow.response import ResponseCurves

    schema, table, pipe, p = _mlp_setup(tmp_path)
    n = 1000
    choke = [0.15, 0.3, 0.5, 0.7, 0.9]
    fields = list(next(ix for ix in pipe.indexers if ix.column == "field").labels)
    pred = Predictor.load(p, schema, device="cuda", precision="bf16", batch=512)
    res = ResponseCurves(pred).run(table, ["choke", "field"], grids={"choke": choke}, by="well")
    S = 1 + 5 + len(fields)
    assert res["native"] and pred.eng_batch == 512 and res["scored"] == n and res["sums"].shape == (S, 8, 3)
    assert res["grids"]["field"] == fields
    eng = pred.eng
    ids = np.unique(np.asarray(table["well"]).astype(str), return_inverse=True)[1]

    def host_fed(tab):  # 1000 rows: a full chunk of 512 and a short one of 488
        Xh = eng.to_input_format(torch.from_numpy(pipe.features(tab))).to(DEV)
        out = torch.cat([eng.forward(Xh[a : a + 512]).clone() for a in (0, 512)]).cpu().numpy()
        return _host_groups(out, ids, 8, pipe.y_std, pipe.y_mean)

    want = [host_fed(table)] + [host_fed(_replaced(table, "choke", np.float32(v))) for v in choke] + \
           [host_fed(_replaced(table, "field", v)) for v in fields]
    _check_slots(res["sums"], want, "native MLP passes vs host-fed engine")
    # a column the first layer does not read: the baseline bit for bit, delta exactly 0
    for s in range(6, S):
        assert np.array_equal(res["sums"][s].view(np.int64), res["sums"][0].view(np.int64))
    fcells = [d for d in res["curves"] if d["column"] == "field"]
    assert len(fcells) == len(fields) * 9 and all(d["delta"] == 0.0 for d in fcells)
    assert any(d["delta"] != 0.0 for d in res["curves"] if d["column"] == "choke")

    # the assembled table in pieces of 512 rows
    pieced = ResponseCurves(pred, piece_rows=512).run(table, ["choke", "field"], grids={"choke": choke}, by="well")
    assert np.array_equal(pieced["sums"], res["sums"])  # the same launches on the same rows

    # the curves against the fp32 oracle on the same grids
    cpu = Predictor.load(p, schema, device="cpu", precision="fp32")
    ora = ResponseCurves(cpu).run(table, ["choke", "field"], grids={"choke": choke}, by="well")
    a = np.asarray([d["mean_prediction"] for d in res["curves"]])
    b = np.asarray([d["mean_prediction"] for d in ora["curves"]])
    rel = float(np.linalg.norm(a - b) / np.linalg.norm(b))
    print("native bf16 vs fp32 oracle, rel-L2 over all mean_prediction cells:", rel)
    assert not ora["native"] and len(a) == S * 9 and rel < 2e-2


def test_wide_tables_take_the_host_path_with_the_native_engines(tmp_path, monkeypatch):
    """Above the device assembly's width limit the features are built on the host and the native
    engines score them: the same sums as the device pass loop."""
    from wellflow.models.lstm import LSTMRegressor
    from wellflow.predict import Predictor
    from wellflow.response import ResponseCurves

    schema, table, pipe, pm = _mlp_setup(tmp_path, blind=False)
    torch.manual_seed(0)
    pl = str(tmp_path / "models" / "lstm.mdl")
    save_mdl(pl, "lstm", registry.keras_layers("lstm", LSTMRegressor(18, 128)),
             {"features": pipe.state(), "job": {"seq_len": 8, "group_col": "well", "hidden": 128}})
    kw = dict(grids={"choke": [0.2, 0.8], "field": ["F1", "never"]}, by="well")
    note = lambda s: None  # noqa: E731
    for path, batch, scored in ((pm, 512, 1000), (pl, 64, 8 * (125 - 7))):
        dev = ResponseCurves(Predictor.load(path, schema, device="cuda", precision="bf16", batch=batch), note=note).run(
            table, ["field", "choke"], **kw)
        with monkeypatch.context() as m:
            m.setattr("wellflow.ops.native.ASSEMBLE_MAX_F", 8)
            job = ResponseCurves(Predictor.load(path, schema, device="cuda", precision="bf16", batch=batch), note=note)
            host = job.run(table, ["field", "choke"], **kw)
        assert dev["native"] and host["native"] and dev["scored"] == host["scored"] == scored
        assert dev["sums"].shape == (5, 8, 3) and np.isfinite(dev["sums"]).all()
        # the bound of test_group_sums between two summations; only the sums are at hand here, and
        # |sum v| <= sum |v|, so n 2^-52 |sum v| asks no less than n 2^-52 sum |v|
        n, s1, s2 = host["sums"][..., 0], host["sums"][..., 1], host["sums"][..., 2]
        assert np.array_equal(dev["sums"][..., 0], n)
        e1, e2 = np.abs(dev["sums"][..., 1] - s1), np.abs(dev["sums"][..., 2] - s2)
        print("host-assembled vs device pass loop: max err", e1.max(), e2.max(), "bounds",
              (n * EPS * np.abs(s1)).min(), (n * EPS * s2).min())
        assert (e1 <= n * EPS * np.abs(s1)).all() and (e2 <= n * EPS * s2).all()


# ------------------------------------------------------------------ 4. the native LSTM passes
def test_native_lstm_passes_equal_host_gathered_windows(tmp_path):
    from wellflow.models.lstm import LSTMRegressor
    from wellflow.predict import Predictor
    from wellflow.response import ResponseCurves

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
    x0 = [-2.0, 1.0, 4.0]
    res = ResponseCurves(pred).run(table, ["well", "x0"], grids={"x0": x0}, by="well")
    eng = pred.eng
    assert res["native"] and pred.eng_batch == 64 and eng.H == H and eng.T == T
    assert res["scored"] == 129 and res["rows"] == n  # three chunks of 64: the last holds one window
    wells = list(pipe.indexers[0].labels)
    assert res["grids"]["well"] == wells and res["groups"] == ["W0", "W1", "W2"] and res["sums"].shape == (7, 3, 3)
    ids = np.unique(table["well"].astype(str), return_inverse=True)[1]
    order = np.argsort(ids, kind="stable")
    stable = take(table, order)
    starts = np.asarray(window_starts(n, T, ids[order]))
    wid = ids[order][starts + T - 1]  # each window's group is its last row's well
    assert np.bincount(wid).tolist() == [43, 43, 43]

    def host_fed(tab):
        X = pipe.features(tab)
        Xw = torch.from_numpy(X[starts[:, None] + np.arange(T)[None, :]]).to(DEV)
        out = torch.cat([eng.forward(Xw[a : a + 64]).clone() for a in range(0, 129, 64)]).cpu().numpy()
        return _host_groups(out, wid, 3, 1.0, 0.0)

    want = [host_fed(stable)] + [host_fed(_replaced(stable, "well", v)) for v in wells] + \
           [host_fed(_replaced(stable, "x0", np.float32(v))) for v in x0]
    _check_slots(res["sums"], want, "native LSTM passes vs host-gathered windows")
    assert not np.array_equal(res["sums"][1], res["sums"][0]) and not np.array_equal(res["sums"][4], res["sums"][0])
    assert eng.persistent_error() == 0, eng.persistent_stats()


# ------------------------------------------------------------------ 5. end to end
def test_train_then_response_job_on_the_gpu(tmp_path):
    from wellflow.response import CSV_COLUMNS, run_response
    from wellflow.train.job import run_job

    sp = str(tmp_path) + "/"
    out = run_job("mlp", [NAMES, TYPES, "flow", sp, "--max-steps", "20", "--synth-wells", "4", "--synth-steps", "200",
                          "--verbose", "0"], **QUIET)
    assert out["native"]
    schema = parse_schema(NAMES, TYPES)
    table = load_table("synth", schema, synth_wells=4, synth_steps=200, seed=42)
    path = str(tmp_path / "data.csv")
    write_csv(table, path, columns=NAMES.split(","))
    res = run_response("mlp", [NAMES, TYPES, "flow", sp, path, "--columns", "choke", "--points", "5", "--by", "well"], **QUIET)
    assert res["native"] and res["scored"] == 800 and res["out"] == sp + "response/mlp.csv"
    with open(res["out"], newline="") as f:
        rows = list(csv.reader(f))
    assert tuple(rows[0]) == CSV_COLUMNS == ("column", "kind", "value", "group", "rows", "mean_prediction",
                                             "std_prediction", "delta")
    body = rows[1:]
    assert len(body) == (1 + 5) * (1 + 4)
    vals = np.asarray([[float(v) for v in r[4:]] for r in body])
    assert np.isfinite(vals).all()
    for b in range(6):
        blk = vals[b * 5 : b * 5 + 5]
        assert blk[0, 0] == 800 and blk[1:, 0].sum() == 800  # the overall cell, and the groups of a pass
    assert (vals[:5, 3] == 0.0).all() and [r[1] for r in body[:5]] == ["baseline"] * 5
    assert [r[0] for r in body[5:]] == ["choke"] * 25 and [r[1] for r in body[5:]] == ["continuous"] * 25
