"""Set points on the GPU: the per-row bracket rule (csrc/score.hip solve_step) against the numpy
rule bit for bit, the assembly kernel's per-row values (perm_values, csrc/features.hip) bit for bit,
and the native pass loops of wellflow/setpoint.py against a replay of the numpy rule over the same
engines fed from the host."""
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
NAN = float("nan")
STATE = ("lo", "hi", "best_x", "xq", "f_lo", "f_hi", "best_r", "bracket")


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


# ------------------------------------------------------------------ 1. solve_step
GRID5 = np.asarray([1.0, 2.5, 3.0, 7.0, 8.0], np.float32)
PLANTED = [  # residuals of a first scan, 4 scans and 3 refines (tests/test_setpoint_cpu.py)
    [0, 1, 2, 3, 4, -1, 1, -1],          # 0: residual exactly 0 at the first grid point
    [-2, -1, 0, 1, 2, 1, -1, 1],         # 1: ... at a middle one
    [-4, -3, -2, -1, 0, -1, 1, 0],       # 2: ... at the last one (and at a refine pass)
    [-1, 1, -1, 1, 2, -1, -1, 1],        # 3: two crossings: the first wins
    [5, 3, 2, 3, 4, -9, -9, -9],         # 4: no crossing
    [3, 2, 4, 2, 5, 1, 1, 1],            # 5: equal misses: the first wins
    [-3, NAN, -1, 1, 2, 1, NAN, -1],     # 6: NaN at one scan pass and at one refine pass
    [NAN, 3, 2, 1, 2, 0, 0, 0],          # 7: NaN first: the first number replaces it
    [NAN] * 8,                           # 8: all NaN
    [2, 1, NAN, -1, 1, 1, 1, 1],         # 9: a NaN between the two sides: no bracket across it
    [0, 0, 0, 0, 0, 0, 0, 0],            # 10: zero everywhere
]


def planted(m, seed, ys=2.0, sh=0.5):
    """Predictions of 8 passes over m rows and the wanted values: random rows and, spread over
    the vector (as many as fit), the planted sequences, whose residuals are exact for ys, sh."""
    rng = np.random.default_rng(seed)
    want = (rng.normal(size=m) * 2).astype(np.float32)
    p = ((want[None, :] - sh) / ys + rng.normal(size=(8, m))).astype(np.float32)
    at = [int(i) for i in np.linspace(0, m - 1, len(PLANTED))] if m >= len(PLANTED) else list(range(m))
    for i, seq in zip(at, PLANTED):
        want[i] = np.float32(3.0)
        p[:, i] = [np.float32((3.0 + v - sh) / ys) for v in seq]
    return [p[t].copy() for t in range(8)], want, at


def run_host(passes, want, ys, sh):
    from wellflow.setpoint import FIRST, REFINE, SCAN, new_state, solve_step_host

    xs, fs, status = new_state(len(want))
    for t, p in enumerate(passes):
        solve_step_host(p, want, ys, sh, FIRST if t == 0 else (SCAN if t < 5 else REFINE), GRID5[t] if t < 5 else None,
                        xs, fs, status)
    return xs, fs, status


def run_device(passes, want, ys, sh, watch=False):
    from wellflow.ops.native import SOLVE_FIRST, SOLVE_REFINE, SOLVE_SCAN, solve_step

    m = len(want)
    xs = torch.full((4, m), NAN, dtype=torch.float32, device=DEV)  # a first scan reads no state
    fs = torch.full((3, m), NAN, dtype=torch.float64, device=DEV)
    status = torch.full((m,), 7, dtype=torch.int32, device=DEV)
    wd, grid = torch.from_numpy(want).to(DEV), torch.from_numpy(GRID5).to(DEV)
    for t, p in enumerate(passes):
        pd = torch.from_numpy(p).to(DEV)
        if watch and 0 < t < 5:
            got = status == 1
            before = (xs[:, got].clone(), fs[:, got].clone())
        mode = SOLVE_FIRST if t == 0 else (SOLVE_SCAN if t < 5 else SOLVE_REFINE)
        solve_step(pd, wd, ys, sh, mode, grid[t : t + 1] if t < 5 else None, xs, fs, status)
        if watch and 0 < t < 5:  # a bracketed row is left alone by a later scan
            assert torch.equal(xs[:, got].view(torch.int32), before[0].view(torch.int32))
            assert torch.equal(fs[:, got].view(torch.int64), before[1].view(torch.int64))
            assert bool((status[got] == 1).all())
    return xs.cpu().numpy(), fs.cpu().numpy(), status.cpu().numpy()


@pytest.mark.parametrize("m", [1, 63, 257, 70001])
def test_solve_step_equals_the_numpy_rule(m):
    for ys, sh in ((2.0, 0.5), (37.25 + 1.0 / 3.0, 101.0 / 7.0)):
        passes, want, at = planted(m, m)
        xs, fs, status = run_device(passes, want, ys, sh, watch=True)
        wxs, wfs, wst = run_host(passes, want, ys, sh)
        for r in range(4):
            assert same_bits(xs[r], wxs[r]), (STATE[r], ys)
        for r in range(3):
            assert same_bits(fs[r], wfs[r]), (STATE[4 + r], ys)
        assert np.array_equal(status, wst), ys
        xs2, fs2, st2 = run_device(passes, want, ys, sh)  # two runs are bitwise equal
        assert same_bits(xs2, xs) and same_bits(fs2, fs) and np.array_equal(st2, status)
    if m < len(PLANTED):
        return
    # the planted rows by hand (their residuals are exact for ys = 2, sh = 0.5)
    passes, want, at = planted(m, m)
    xs, fs, status = run_device(passes, want, 2.0, 0.5)
    assert status[at].tolist() == [1, 1, 1, 1, 0, 0, 1, 0, 0, 1, 1]
    assert (xs[0, at[2]], xs[1, at[2]], fs[0, at[2]], fs[1, at[2]]) == (7.5, 7.625, -1.0, 0.0)
    assert (xs[2, at[5]], fs[2, at[5]]) == (2.5, 2.0) and (xs[2, at[4]], fs[2, at[4]]) == (3.0, 2.0)
    # a NaN stays in its row: every other row equals a run without the NaN rows' predictions
    nan_rows = [at[6], at[7], at[8], at[9]]
    clean = [p.copy() for p in passes]
    for p in clean:
        p[nan_rows] = 1.0
    cxs, cfs, cst = run_device(clean, want, 2.0, 0.5)
    keep = np.ones(m, bool)
    keep[nan_rows] = False
    assert not np.isnan(cfs).any() and np.isnan(fs[:, at[8]]).all()
    assert same_bits(cxs[:, keep], xs[:, keep]) and same_bits(cfs[:, keep], fs[:, keep]) and np.array_equal(cst[keep], status[keep])


def test_solve_step_refusals():
    from wellflow.ops.native import SOLVE_FIRST, SOLVE_REFINE, SOLVE_SCAN, solve_step

    m = 10
    p, w = torch.zeros(m, device=DEV), torch.zeros(m, device=DEV)
    xs = torch.zeros((4, m), device=DEV)
    fs = torch.zeros((3, m), dtype=torch.float64, device=DEV)
    st = torch.zeros(m, dtype=torch.int32, device=DEV)
    g = torch.ones(1, device=DEV)
    with pytest.raises(TypeError, match="p must be a float32"):
        solve_step(p.double(), w, 1.0, 0.0, SOLVE_FIRST, g, xs, fs, st)
    with pytest.raises(TypeError, match="want must be a float32"):
        solve_step(p, w.cpu().numpy(), 1.0, 0.0, SOLVE_FIRST, g, xs, fs, st)
    with pytest.raises(ValueError, match="must be equal vectors"):
        solve_step(p, w[:9], 1.0, 0.0, SOLVE_FIRST, g, xs, fs, st)
    with pytest.raises(ValueError, match=r"no predictions \(M < 1\)"):
        solve_step(p[:0], w[:0], 1.0, 0.0, SOLVE_FIRST, g, xs[:, :0], fs[:, :0], st[:0])
    with pytest.raises(ValueError, match="mode 3 is not"):
        solve_step(p, w, 1.0, 0.0, 3, g, xs, fs, st)
    with pytest.raises(TypeError, match="xs must be a torch.float32"):
        solve_step(p, w, 1.0, 0.0, SOLVE_FIRST, g, xs.double(), fs, st)
    with pytest.raises(TypeError, match="fs must be a torch.float64"):
        solve_step(p, w, 1.0, 0.0, SOLVE_FIRST, g, xs, fs.float(), st)
    with pytest.raises(ValueError, match=r"xs must be \[4\]\[10\]"):
        solve_step(p, w, 1.0, 0.0, SOLVE_FIRST, g, xs[:3], fs, st)
    with pytest.raises(ValueError, match=r"fs must be \[3\]\[10\]"):
        solve_step(p, w, 1.0, 0.0, SOLVE_FIRST, g, xs, fs[:, :9], st)
    with pytest.raises(TypeError, match="status must be an int32"):
        solve_step(p, w, 1.0, 0.0, SOLVE_FIRST, g, xs, fs, st.long())
    with pytest.raises(ValueError, match=r"status must be \[10\]"):
        solve_step(p, w, 1.0, 0.0, SOLVE_FIRST, g, xs, fs, st[:9])
    with pytest.raises(ValueError, match="on one GPU"):
        solve_step(p, w.cpu(), 1.0, 0.0, SOLVE_FIRST, g, xs, fs, st)
    with pytest.raises(ValueError, match="on one GPU"):
        solve_step(p.cpu(), w.cpu(), 1.0, 0.0, SOLVE_FIRST, g.cpu(), xs.cpu(), fs.cpu(), st.cpu())
    wide = torch.zeros((4, 2 * m), device=DEV)
    with pytest.raises(ValueError, match="xs must be contiguous"):
        solve_step(p, w, 1.0, 0.0, SOLVE_FIRST, g, wide[:, ::2], fs, st)
    with pytest.raises(ValueError, match="p must be contiguous"):
        solve_step(wide[0, ::2], w, 1.0, 0.0, SOLVE_FIRST, g, xs, fs, st)
    with pytest.raises(TypeError, match="grid_x must be a float32 tensor"):
        solve_step(p, w, 1.0, 0.0, SOLVE_SCAN, None, xs, fs, st)
    with pytest.raises(ValueError, match="grid_x must be one contiguous element"):
        solve_step(p, w, 1.0, 0.0, SOLVE_SCAN, torch.ones(2, device=DEV), xs, fs, st)
    with pytest.raises(ValueError, match="grid_x must be one contiguous element"):
        solve_step(p, w, 1.0, 0.0, SOLVE_SCAN, g.cpu(), xs, fs, st)
    with pytest.raises(ValueError, match="grid_x must be None"):
        solve_step(p, w, 1.0, 0.0, SOLVE_REFINE, g, xs, fs, st)
    with pytest.raises(ValueError, match=r"p overlaps the state \(xs\)"):
        solve_step(xs[3], w, 1.0, 0.0, SOLVE_REFINE, None, xs, fs, st)
    with pytest.raises(ValueError, match=r"want overlaps the state \(xs\)"):
        solve_step(p, xs[0], 1.0, 0.0, SOLVE_FIRST, g, xs, fs, st)
    assert (xs == 0).all().item() and (fs == 0).all().item() and (st == 0).all().item()  # nothing was launched
    # the binding refuses the same on its own (a direct caller): still before any launch
    from wellflow.ops.native import lib

    with pytest.raises(RuntimeError, match="overlap the state"):
        lib().solve_step(xs[3], w, 1.0, 0.0, 2, None, xs, fs, st)
    with pytest.raises(RuntimeError, match="mode 5 outside"):
        lib().solve_step(p, w, 1.0, 0.0, 5, g, xs, fs, st)
    with pytest.raises(RuntimeError, match="grid_x must be one"):
        lib().solve_step(p, w, 1.0, 0.0, 0, None, xs, fs, st)
    with pytest.raises(RuntimeError, match=r"xs must be a contiguous fp32 \[4\]\[10\]"):
        lib().solve_step(p, w, 1.0, 0.0, 0, g, xs[:3], fs, st)
    assert (xs == 0).all().item() and (fs == 0).all().item()


# ------------------------------------------------------------------ 2. per-row values in the assembly
# the column sets, sizes and formats of tests/test_explain_gpu.py
N_MAX = 4099
SIZES = [1, 63, 64, 65, 1000, N_MAX]
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


def _values(n, seed):
    """Finite float32 values with 1e-3 <= |v| <= 1e4, one per row."""
    rng = np.random.default_rng(seed)
    return (10.0 ** rng.uniform(-3.0, 4.0, size=n) * rng.choice([-1.0, 1.0], size=n)).astype(np.float32)


def _bits(t):
    t = t.cpu()
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("key", list(COLUMN_SETS))
def test_perm_values_assembly_is_bit_exact(key, n):
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
    C, Q = codes.shape[0], (cont.shape[0] if cont.ndim == 2 else 0)
    res = ResidentColumns(codes, cont, off, size, mean, std, F, DEV)
    host32 = torch.from_numpy(pipe.features(sub))
    formats = ((torch.float32, F, host32), (torch.bfloat16, Fp, NativeMLP.to_input_format(stub, host32)))
    # the plain and the perm_col launches through the new call shape equal the host pipeline as before
    perm = np.random.default_rng(n + C).permutation(n)
    pd = torch.from_numpy(perm.astype(np.int32)).to(DEV)
    for dt, ld, want in formats:
        out = torch.full((n, ld), NAN, dtype=dt, device=DEV)
        res.assemble(dt, out=out)
        assert torch.equal(_bits(out), _bits(want)), (key, n, dt, "plain")
        for k in {0, C + Q - 1}:
            t2 = dict(sub)
            t2[names[k]] = np.asarray(sub[names[k]])[perm]
            w32 = torch.from_numpy(pipe.features(t2))
            got = res.assemble(dt, perm=pd, perm_col=k)
            assert torch.equal(_bits(got), _bits(w32 if dt == torch.float32 else NativeMLP.to_input_format(stub, w32))), (key, n, dt, k)
    if Q == 0:
        return
    vals = _values(n, 17 * n + Q)
    vd = torch.from_numpy(vals).to(DEV)
    index = {"identity": np.arange(n), "reversed": np.arange(n)[::-1].copy()}
    for k in sorted({C, C + Q - 1}):  # the first and the last continuous column
        for what, ix in index.items():
            xd = torch.from_numpy(ix.astype(np.int32)).to(DEV)
            t2 = dict(sub)
            t2[names[k]] = vals[ix]
            cont2 = cont.copy()
            cont2[k - C] = vals[ix]
            want32 = torch.from_numpy(pipe.features(t2))                                       # (a) the host pipeline
            for dt, ld, _ in formats:
                out = torch.full((n, ld), NAN, dtype=dt, device=DEV)                           # unwritten padding would show
                got = res.assemble(dt, perm=xd, perm_col=k, perm_values=vd, out=out)
                assert got.data_ptr() == out.data_ptr()
                want = want32 if dt == torch.float32 else NativeMLP.to_input_format(stub, want32)
                assert torch.equal(_bits(out), _bits(want)), (key, n, k, what, dt)
                over = assemble_features(codes, cont2, off, size, mean, std, F, dt, DEV)      # (b) the plain kernel
                assert torch.equal(_bits(out), _bits(over)), (key, n, k, what, dt)


@pytest.mark.parametrize("key", ["c3_17_q7", "c40_q9"])
def test_perm_values_of_a_piece_and_clamped_indices(key):
    """Output rows [64, 200) of N = 1000 read their values through ident[64:200] from all 1000
    values; indices outside the vector are clamped into it, not read."""
    from wellflow.ops.native import ResidentColumns, assemble_features

    pipe, table = _reference(key)
    n, a, b = 1000, 64, 200
    codes, cont = pipe.raw_columns(take(table, np.arange(n)))
    off, size = pipe.block_spec()
    mean, std = pipe.scale()
    res = ResidentColumns(codes, cont, off, size, mean, std, pipe.n_features, DEV)
    C, Q = res.C, res.Q
    vals = _values(n, 9)
    vd = torch.from_numpy(vals).to(DEV)
    ident = torch.arange(n, dtype=torch.int32, device=DEV)
    rev = torch.arange(n - 1, -1, -1, dtype=torch.int32, device=DEV)
    wild = np.random.default_rng(5).integers(-3 * n, 4 * n, size=n)
    wild[:4] = [-1, n, -2 ** 31, 2 ** 31 - 1]
    assert (wild < 0).sum() > 100 and (wild >= n).sum() > 100
    wd = torch.from_numpy(wild.astype(np.int32)).to(DEV)
    for k in (C, C + Q - 1):
        for dt in (torch.float32, torch.bfloat16):
            for ix in (ident, rev):  # rev[a:b] reads rows (n - b, n - a]: outside the piece
                whole = res.assemble(dt, perm=ix, perm_col=k, perm_values=vd)
                out = torch.full((b - a, whole.shape[1]), NAN, dtype=dt, device=DEV)
                res.assemble(dt, rows=(a, b), perm=ix[a:b], perm_col=k, perm_values=vd, out=out)
                assert torch.equal(_bits(out), _bits(whole[a:b])), (k, dt)
            cont2 = cont.copy()
            cont2[k - C] = vals
            over = assemble_features(codes, cont2, off, size, mean, std, pipe.n_features, dt, DEV)
            assert torch.equal(_bits(res.assemble(dt, rows=(a, b), perm=ident[a:b], perm_col=k, perm_values=vd)), _bits(over[a:b]))
            cont2[k - C] = vals[np.clip(wild, 0, n - 1)]  # the values of the clamped host gather
            over = assemble_features(codes, cont2, off, size, mean, std, pipe.n_features, dt, DEV)
            assert torch.equal(_bits(res.assemble(dt, perm=wd, perm_col=k, perm_values=vd)), _bits(over)), (k, dt)
            got = res.assemble(dt, rows=(a, b), perm=wd[a:b], perm_col=k, perm_values=vd)
            assert torch.equal(_bits(got), _bits(over[a:b])), (k, dt)


def test_perm_values_refusals_come_from_the_host():
    from wellflow.ops.native import ResidentColumns, column_masks, lib

    pipe, table = _reference("c3_17_q7")
    n = 130
    codes, cont = pipe.raw_columns(take(table, np.arange(n)))
    res = ResidentColumns(codes, cont, *pipe.block_spec(), *pipe.scale(), pipe.n_features, DEV)
    ident = torch.arange(n, dtype=torch.int32, device=DEV)
    vals = torch.ones(n, device=DEV)
    mask = column_masks([[0, 3]], 9, DEV)[0]
    one = torch.zeros(1, dtype=torch.float32, device=DEV)
    with pytest.raises(ValueError, match=r"needs a continuous perm_col.*got 1 \(a categorical column\)"):
        res.assemble(torch.float32, perm=ident, perm_col=1, perm_values=vals)
    with pytest.raises(ValueError, match="needs a continuous perm_col"):
        res.assemble(torch.float32, perm=ident, perm_col=9, perm_values=vals)
    with pytest.raises(ValueError, match=r"not combined with a set of permuted columns \(col_set\)"):
        res.assemble(torch.float32, perm=ident, col_set=mask, perm_values=vals)
    with pytest.raises(ValueError, match="not combined with a constant"):
        res.assemble(torch.float32, perm_values=vals, const_col=4, const_value=one)
    with pytest.raises(ValueError, match="goes together with perm and perm_col"):
        res.assemble(torch.float32, perm_values=vals)
    with pytest.raises(TypeError, match="perm_values must be float32"):
        res.assemble(torch.float32, perm=ident, perm_col=4, perm_values=vals.double())
    with pytest.raises(ValueError, match=r"holds \(129,\) values for the table's 130 rows"):
        res.assemble(torch.float32, perm=ident, perm_col=4, perm_values=vals[:129])
    with pytest.raises(ValueError, match="values for the table's 130 rows"):  # ALL rows, also for a piece
        res.assemble(torch.float32, rows=(0, 64), perm=ident[:64], perm_col=4, perm_values=vals[:64])
    with pytest.raises(ValueError, match="perm_values must be a tensor on"):
        res.assemble(torch.float32, perm=ident, perm_col=4, perm_values=vals.cpu())
    with pytest.raises(ValueError, match="values for the table's 130 rows"):
        res.assemble(torch.float32, perm=ident, perm_col=4, perm_values=torch.ones(2 * n, device=DEV)[::2])
    with pytest.raises(ValueError, match="for 130 rows"):
        res.assemble(torch.float32, perm=ident[:129], perm_col=4, perm_values=vals)
    # the binding refuses the same on its own (a direct caller): still before any launch
    out = torch.empty((n, 27), device=DEV)
    args = (res.codes, res.cont, res.off, res.size, res.mean, res.std, 0, n, 27, out)
    with pytest.raises(RuntimeError, match="needs a continuous perm_col"):
        lib().assemble_features(*args, 1, ident, perm_values=vals)
    with pytest.raises(RuntimeError, match="not combined with a set"):
        lib().assemble_features(*args, -1, ident, set_mask=mask, perm_values=vals)
    with pytest.raises(RuntimeError, match="not combined with a constant"):
        lib().assemble_features(*args, -1, None, 4, one, perm_values=vals)
    with pytest.raises(RuntimeError, match="goes together with perm and perm_col"):
        lib().assemble_features(*args, -1, None, perm_values=vals)
    with pytest.raises(RuntimeError, match="perm_values must be a contiguous float32 vector"):
        lib().assemble_features(*args, 4, ident, perm_values=vals.double())
    with pytest.raises(RuntimeError, match="perm_values holds 129 values"):
        lib().assemble_features(*args, 4, ident, perm_values=vals[:129])


# ------------------------------------------------------------------ 3. the native jobs
def replay(score, want, grid, refine, ys, sh):
    """The numpy rule over ``score(kind, x)``: the fp32 outputs of the table as it is (kind None),
    with the column constant (``"const"``, a float32) or set per row (``"rows"``, float32 [M])."""
    from wellflow.setpoint import FIRST, REFINE, SCAN, finish_host, new_state, solve_step_host

    p0 = np.asarray(score(None, None))
    xs, fs, status = new_state(len(p0))
    for g, v in enumerate(grid):
        solve_step_host(np.asarray(score("const", np.float32(v))), want, ys, sh, FIRST if g == 0 else SCAN, v, xs, fs, status)
    for _ in range(refine):
        solve_step_host(np.asarray(score("rows", xs[3].copy())), want, ys, sh, REFINE, None, xs, fs, status)
    out = finish_host(xs, fs, status)
    out["prediction"] = p0.astype(np.float64) * ys + sh
    return out


def _same(res, want, names=STATE + ("setpoint", "miss", "prediction")):
    for name in names:
        assert same_bits(np.asarray(res[name]), np.asarray(want[name])), name


@pytest.fixture(scope="module")
def fitted(tmp_path_factory):
    """An MLP (18 -> 256 -> 256 -> 1) fitted for a few hundred steps on the synthetic table (8 wells
    x 125 steps), and an LSTM with drawn weights on the same pipeline."""
    from wellflow.models.lstm import LSTMRegressor
    from wellflow.models.mlp import MLPRegressor

    d = tmp_path_factory.mktemp("setpoint_gpu")
    schema = parse_schema(NAMES, TYPES)
    table = load_table("synth", schema, synth_wells=8, synth_steps=125, seed=3)
    pipe = FeaturePipeline(schema, "flow", standardize_target=True).fit(table)
    assert pipe.n_features == 18  # 8 well columns + 3 field columns + 7 continuous
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
    return dict(schema=schema, table=table, pipe=pipe, mlp=pm, lstm=pl)


def _mlp_host_fed(eng, pipe, table, column):
    def score(kind, x):  # 1000 rows: a full chunk of 512 and a short one of 488
        t2 = dict(table)
        if kind == "const":
            t2[column] = np.full(1000, x, np.float32)
        elif kind == "rows":
            t2[column] = np.asarray(x, np.float32)
        Xh = eng.to_input_format(torch.from_numpy(pipe.features(t2))).to(DEV)
        return torch.cat([eng.forward(Xh[a : a + 512]).clone() for a in (0, 512)]).cpu().numpy()

    return score


# Measured on an MI355X for this file's fixed seeds (profiles/r7/setpoint/README.md) and asserted at
# twice the recorded worst case: a step of the bf16 staircase can move a crossing by one refine
# interval either way, and a row whose residual comes within the bf16 error of zero at a grid point
# can bracket in another cell, or not at all.
ORACLE_STATUS_DISAGREE = 2 * 3          # rows of 1000 whose status differs (measured: 3)
ORACLE_SETPOINT_STEPS = 2 * 0.07953     # max |setpoint_native - setpoint_oracle| / grid step over the rows bracketed
#                                         in both (measured: 0.07953 over 909 rows, median 0.0051)


def test_native_mlp_job_equals_host_fed_engine(fitted, monkeypatch):
    from wellflow.predict import Predictor
    from wellflow.setpoint import SetPoint

    schema, table, pipe = fitted["schema"], fitted["table"], fitted["pipe"]
    want = np.asarray(table["flow"], np.float32)
    G, S = 9, 6
    pred = Predictor.load(fitted["mlp"], schema, device="cuda", precision="bf16", batch=512)
    res = SetPoint(pred, points=G, refine=S).run(table, "choke", want)
    assert res["native"] and pred.eng_batch == 512 and res["scored"] == 1000 and res["passes"] == 1 + G + S
    ys, sh = float(pipe.y_std), float(pipe.y_mean)
    ref = replay(_mlp_host_fed(pred.eng, pipe, table, "choke"), want, res["grid"], S, ys, sh)
    _same(res, ref)
    got = res["bracket"] == 1
    print("native MLP: bracketed", int(got.sum()), "of 1000; median width", res["median_width"])
    assert 100 < got.sum() < 1000 and res["bracketed"] + res["open"] == 1000
    step = float(np.diff(res["grid"].astype(np.float64)).max())
    assert (np.abs(res["hi"] - res["lo"])[got] <= step / 2 ** S + S * 2.0 ** -24 * np.abs(res["hi"][got])).all()

    # the assembled table in pieces of 512 rows (a piece reads its values from all 1000)
    pieced = SetPoint(pred, points=G, refine=S, piece_rows=512).run(table, "choke", want)
    _same(pieced, res)

    # a table wider than the device assembly's limit: host rows, the native engine, solve_step on the device
    notes = []
    with monkeypatch.context() as m:
        m.setattr("wellflow.ops.native.ASSEMBLE_MAX_F", 8)
        wide = SetPoint(Predictor.load(fitted["mlp"], schema, device="cuda", precision="bf16", batch=512), points=G,
                        refine=S, note=notes.append).run(table, "choke", want)
    assert wide["native"] and len(notes) == 1 and "once per refine pass" in notes[0]
    _same(wide, res)

    # against the fp32 oracle: the status agreement and the setpoint difference in grid steps
    cpu = Predictor.load(fitted["mlp"], schema, device="cpu", precision="fp32")
    ora = SetPoint(cpu, points=G, refine=S).run(table, "choke", want)
    agree = res["bracket"] == ora["bracket"]
    both = (res["bracket"] == 1) & (ora["bracket"] == 1)
    diff = np.abs(res["setpoint"] - ora["setpoint"])[both] / step
    print("vs fp32 oracle: status disagrees in", int((~agree).sum()), "of 1000 rows; bracketed in both", int(both.sum()),
          "; setpoint difference / grid step: max", float(diff.max()), "median", float(np.median(diff)))
    assert both.sum() > 500
    assert (~agree).sum() <= ORACLE_STATUS_DISAGREE
    assert float(diff.max()) <= ORACLE_SETPOINT_STEPS


def test_native_lstm_job_scans_only(fitted):
    from wellflow.predict import Predictor
    from wellflow.setpoint import SetPoint

    schema, table, pipe = fitted["schema"], fitted["table"], fitted["pipe"]
    n, T = 1000, 8
    sub = take(table, np.arange(0, n, 5))  # 200 rows, 25 per well: 8 x 18 = 144 windows, three launches of 64
    n = 200
    pred = Predictor.load(fitted["lstm"], schema, device="cuda", precision="bf16", batch=64)
    # wanted: halfway between the fp32 oracle's outputs at two chokes, so most windows have a crossing
    from wellflow.scoring import ConstantColumn
    from wellflow.whatif import input_columns, scorer_for

    cpu = Predictor.load(fitted["lstm"], schema, device="cpu", precision="fp32")
    oracle = scorer_for(cpu, sub, "set-point")
    k = [c for c, _ in input_columns(cpu)].index("choke")
    mid = 0.5 * (np.asarray(oracle.predict(ConstantColumn(k, np.float32(20.0)))).astype(np.float64) +
                 np.asarray(oracle.predict(ConstantColumn(k, np.float32(50.0)))).astype(np.float64))
    want = np.zeros(n, np.float32)
    want[oracle.rows] = (mid * oracle.y_scale + oracle.y_shift).astype(np.float32)
    want[oracle.rows[::5]] = np.float32(1e7)  # out of reach: these windows stay open
    notes = []
    grid = [16.0, 24.0, 40.0, 64.0, 32.0]
    res = SetPoint(pred, refine=4, note=notes.append).run(sub, "choke", want, grid=grid)
    eng = pred.eng
    assert res["native"] and pred.eng_batch == 64 and res["scored"] == 144 and res["refine"] == 0 and res["passes"] == 6
    assert len(notes) == 1 and "scan only" in notes[0]
    ids = np.unique(np.asarray(sub["well"]).astype(str), return_inverse=True)[1]
    order = np.argsort(ids, kind="stable")
    stable = take(sub, order)
    starts = np.asarray(window_starts(n, T, ids[order]))
    rows = order[starts + T - 1]
    assert np.array_equal(res["rows"], rows) and np.array_equal(res["wanted"], want[rows].astype(np.float64))

    def host_fed(kind, x):
        t2 = dict(stable)
        if kind == "const":
            t2["choke"] = np.full(n, x, np.float32)
        X = pipe.features(t2)
        Xw = torch.from_numpy(X[starts[:, None] + np.arange(T)[None, :]]).to(DEV)
        return torch.cat([eng.forward(Xw[a : a + 64]).clone() for a in range(0, 144, 64)]).cpu().numpy()

    ref = replay(host_fed, want[rows], np.asarray(grid, np.float32), 0, float(pipe.y_std), float(pipe.y_mean))
    _same(res, ref)
    print("native LSTM: bracketed", res["bracketed"], "of 144")
    assert 0 < res["bracketed"] < 144 and res["open"] >= 29 and res["bracketed"] + res["open"] == 144
    assert eng.persistent_error() == 0, eng.persistent_stats()


# ------------------------------------------------------------------ 4. end to end
def test_train_then_setpoint_job_on_the_gpu(tmp_path):
    from wellflow.predict import Predictor
    from wellflow.scoring import RowValues
    from wellflow.setpoint import run_setpoint
    from wellflow.train.job import run_job
    from wellflow.whatif import input_columns, scorer_for

    sp = str(tmp_path) + "/"
    out = run_job("mlp", [NAMES, TYPES, "flow", sp, "--max-steps", "60", "--synth-wells", "4", "--synth-steps", "200",
                          "--verbose", "0"], **QUIET)
    assert out["native"]
    schema = parse_schema(NAMES, TYPES)
    table = load_table("synth", schema, synth_wells=4, synth_steps=200, seed=42)
    path = str(tmp_path / "data.csv")
    write_csv(table, path, columns=NAMES.split(","))
    lines = []
    res = run_setpoint("mlp", [NAMES, TYPES, "flow", sp, path, "--column", "choke", "--want-column", "flow", "--points", "9",
                               "--refine", "4"], log=lambda s: lines.append(str(s)))
    assert res["native"] and res["scored"] == 800 and res["passes"] == 14
    with open(res["out"], newline="") as f:
        rows = list(csv.reader(f))
    assert res["out"] == sp + "setpoint/mlp.csv" and len(rows) == 801
    assert rows[0] == NAMES.split(",") + ["prediction", "wanted", "setpoint", "status", "lo", "hi", "miss"]
    kinds = [r[13] for r in rows[1:]]
    assert set(kinds) <= {"bracketed", "nearest", "nan"}
    assert res["bracketed"] + res["open"] == 800 and res["bracketed"] == int((res["bracket"] == 1).sum())
    assert kinds == res["status"] and kinds.count("bracketed") == int((res["code"] == 1).sum()) > 0
    assert lines[:3] == ["Rows scored: 800", "Rows bracketed: %d" % res["bracketed"],
                         "Rows without a crossing: %d" % res["open"]]
    print("end to end:", lines)
    # re-scoring at lo / hi reproduces the signs of f_lo / f_hi
    parsed = load_table(path, schema)
    pred = Predictor.load(sp + "models/mlp.mdl", schema, device="cuda", precision="bf16")
    scorer = scorer_for(pred, parsed, "set-point")
    assert scorer.on_device
    want = np.asarray(parsed["flow"], np.float32).astype(np.float64)
    ident = torch.arange(800, dtype=torch.int32, device=pred.device)
    got = res["bracket"] == 1
    k = [c for c, _ in input_columns(pred)].index("choke")
    for end, f in (("lo", "f_lo"), ("hi", "f_hi")):
        vals = torch.from_numpy(res[end].astype(np.float32)).to(pred.device)
        p = scorer.predict(RowValues(k, vals, ident)).cpu().numpy()
        r = p.astype(np.float64) * scorer.y_scale + scorer.y_shift - want
        assert np.array_equal(np.sign(r[got]), np.sign(res[f][got])), end
