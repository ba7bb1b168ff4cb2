"""The fp32 coalition kernel (csrc/mlp_f32_shap.hip) and the exact Shapley job built on it: every coalition's
output float64 bit for bit on the exact lattice, inside the worst-case fp32 bound on random data, phi against
the numpy rule bit for bit, every refusal, and the job through the kernel against the oracle route."""
import numpy as np
import pytest
import torch

from wellflow.models.mlp import MlpLayout, MLPRegressor, NativeMLP
from wellflow.ops.native import lib
from wellflow.shapley_exact import ExactShapley, exact_shapley_host, shapley_weights
from wellflow.train import exact as ex

pytestmark = pytest.mark.gpu
DEV, HID, NAN, U = "cuda", (256, 256), float("nan"), 2.0 ** -24
NAMES = "well,field,t,whp,choke,glr,temp,water_cut,dsp,flow"
TYPES = "string,string,int,float,float,float,float,float,float,float"
_ENG = {}
# (off, size) per picked column. Between them: spans of 1, a span across an 8-feature K step (6 .. 9), across
# a 32-feature slab (30 .. 34), unpicked features before, between and after, K = 1, and K = 12 at F = 33
SPANS = {5: ([(2, 2)], [(1, 1), (3, 1)]),
         33: ([(1 + 2 * c, 1) for c in range(11)] + [(30, 3)],),
         65: ([(6, 4), (30, 5), (64, 1)],),
         264: ([(0, 40), (100, 1), (250, 14)],),
         512: ([(3, 1), (7, 2), (31, 34), (255, 2), (500, 12)], [(511, 1)])}


def _engine(F, flat):
    if F not in _ENG:
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        _ENG[F] = NativeMLP(F, HID, lib().MLP_F32_ROWS * cus + 1, device=DEV)
    _ENG[F].params.copy_(flat.float().to(DEV))
    _ENG[F].sync_weights()
    return _ENG[F]


def _coalitions64(flat, x, xb, spans, chunk=64):
    """float64, on the device: p(S) [2^K][n] of every coalition (the composed row through the plain forward)
    and ep(S), the bound of test_random_data_inside_the_fp32_bound's docstring."""
    F, K = x.shape[1], len(spans)
    ((W1, b1), (W2, b2)), w3, b3 = MlpLayout(F, HID).views(flat.double().to(DEV))
    W1, x, xb, Fp = W1[:, :F], x.double().to(DEV), xb.double().to(DEV), (F + 7) // 8 * 8
    member = torch.zeros(K, F, dtype=torch.float64, device=DEV)
    for c, (o, n) in enumerate(spans):
        member[c, o : o + n] = 1.0
    bits = ((torch.arange(1 << K, device=DEV)[:, None] >> torch.arange(K, device=DEV)) & 1).double()
    ps, eps = [], []
    for a in range(0, 1 << K, chunk):
        own, back = (bits[a : a + chunk] @ member > 0)[:, None, :], ((1 - bits[a : a + chunk]) @ member > 0)[:, None, :]
        z1 = torch.where(back, xb, x) @ W1.t() + b1
        mag = torch.where(back, xb.abs(), torch.where(own, xb.abs() + (x - xb).abs(), x.abs()))  # |x~| + |d_c|, c in S
        e1 = (Fp + K + 3) * U * (b1.abs() + mag @ W1.abs().t())
        h1 = torch.relu(z1)
        h2 = torch.relu(h1 @ W2.t() + b2)
        e2 = e1 @ W2.abs().t() + 257 * U * (h1 @ W2.abs().t() + b2.abs())
        ps.append(h2 @ w3 + b3)
        eps.append(e2 @ w3.abs() + 257 * U * (h2 @ w3.abs() + b3.abs()))
    return torch.cat(ps).cpu(), torch.cat(eps).cpu()


def _run(eng, x, xb, spans, B):
    """shapley_f32 over rows [0, B) of x (cycled): X in a NaN buffer of stride F + 3, phi (row0 = 2, five spare
    columns), p_out (one spare column) and pred from NaN; checks what must stay untouched and the rule."""
    F, K = x.shape[1], len(spans)
    buf = torch.full((B + 3, F + 3), NAN, device=DEV)
    idx = torch.arange(B) % x.shape[0]
    buf[:B, :F] = x[idx].float().to(DEV)
    phi = torch.full((K, B + 5), NAN, dtype=torch.float64, device=DEV)
    pout = torch.full((1 << K, B + 1), NAN, device=DEV)
    before = eng.params.clone()
    eng.pred.fill_(NAN)
    p0, pf = eng.shapley_f32(buf[:B], xb.float().to(DEV), [o for o, _ in spans], [n for _, n in spans], phi, 2, pout)
    assert phi[:, :2].isnan().all() and phi[:, 2 + B:].isnan().all() and pout[:, B].isnan().all()
    assert eng.pred.isnan().all() and torch.equal(eng.params, before)
    got = pout[:, :B].cpu()
    assert torch.equal(p0.cpu(), got[0]) and torch.equal(pf.cpu(), got[-1])
    assert np.array_equal(phi[:, 2 : 2 + B].cpu().numpy(), exact_shapley_host(got.numpy(), K)), f"phi: K={K} B={B}"
    return got, idx


@pytest.mark.parametrize("row0", (False, True))
@pytest.mark.parametrize("F", (5, 33, 65, 264, 512))
def test_lattice_bit_for_bit(F, row0):
    case = ex.exact_mlp_case(F, HID, 300, 100 * F + 303)
    xb = case.x[0] if row0 else torch.zeros(F)
    eng = _engine(F, case.flat)
    for spans in SPANS[F]:
        x = case.x[:9] if len(spans) == 12 else case.x  # 4096 coalitions: fewer distinct rows and smaller batches
        want = _coalitions64(case.flat, x, xb, spans)[0]
        assert torch.equal(want.float().double(), want)  # fp32-representable
        for B in (1, 65, 129) if len(spans) == 12 else (1, 63, 64, 65, eng.B):  # eng.B: a second tile, a one-row tile
            got, idx = _run(eng, x, xb, spans, B)
            assert torch.equal(got, want.float()[:, idx]), f"F={F} K={len(spans)} B={B}"


@pytest.mark.parametrize("F,spans", ((13, [(0, 3), (4, 1), (6, 4), (11, 2)]),
                                     (40, [(1, 2), (5, 6), (12, 1), (20, 15), (36, 1), (38, 2)])))
def test_random_data_inside_the_fp32_bound(F, spans):
    """The bound, from the kernel's operation order (U = 2^-24, Fp = F padded to 8, K columns). d = fl(x - x')
    carries U |d|; D_c is an fp32 sum of at most Fp terms: (Fp + 1) U |d_c| @ |W1_c|^T. z0 is an Fp-term sum
    plus the add of b1: (Fp + 1) U (|x~| @ |W1|^T + |b1|), x~ the row with every picked span at x'. z1(S) adds
    |S| <= K of the D_c, each add rounding the partial sum once. Together, to first order,
    e1(S) = (Fp + K + 3) U (|b1| + |x~| @ |W1|^T + sum_{c in S} |d_c| @ |W1_c|^T). relu is 1-Lipschitz, layer 2
    is a 256-term sum plus b2, the head a 256-term sum plus b3: e2 = e1 @ |W2|^T + 257 U (h1 @ |W2|^T + |b2|),
    ep = e2 @ |w3| + 257 U (h2 @ |w3| + |b3|). No row is excluded: a flipped mask moves the output by no more
    than the error that flipped it."""
    g = torch.Generator().manual_seed(F)
    flat = 0.1 * torch.randn(MlpLayout(F, HID).numel, generator=g)
    x = torch.randn(293, F, generator=g)
    xb = x.mean(0)
    p64, ep = _coalitions64(flat.float(), x.float(), xb.float(), spans)
    got, _ = _run(_engine(F, flat), x, xb, spans, 293)
    err = (got.double() - p64).abs()
    print(f"F={F} K={len(spans)}: worst error/bound {(err / ep).max():.2e}, bound max {ep.max():.2e}, "
          f"median |p| {p64.abs().median():.3f}")
    assert (err <= ep).all()


def _direct(e, x, b, phi, **kw):
    """The binding, called as the wrapper calls it, with one argument replaced."""
    a = dict(off=torch.tensor([0, 4], dtype=torch.int32), size=torch.tensor([2, 1], dtype=torch.int32),
             coef=torch.from_numpy(shapley_weights(2)), scratch=torch.empty(e._C.mlp2_shapley_scratch_floats(64, 2), device=DEV),
             p_out=None)
    a.update(kw)
    e._C.mlp2_shapley_f32(x, 102, 100, b, *e._views(), a["off"], a["size"], a["coef"], a["scratch"], phi, 0,
                          torch.empty(64, device=DEV), torch.empty(64, device=DEV), a["p_out"], 64)


@pytest.mark.parametrize("call,msg", [
    (lambda e, x, b, o: NativeMLP(100, (256, 128), 64, device=DEV).shapley_f32(x, b, [0], [1], o[:1]), r"hidden \(256, 128\)"),
    (lambda e, x, b, o: NativeMLP(513, HID, 64, device=DEV).shapley_f32(x, b, [0], [1], o[:1]), "520 padded input features > 512"),
    (lambda e, x, b, o: e.shapley_f32(x.bfloat16(), b, [0, 4], [2, 1], o), "contiguous fp32"),
    (lambda e, x, b, o: e.shapley_f32(x, b.cpu(), [0, 4], [2, 1], o), "baseline is on cpu"),
    (lambda e, x, b, o: e.shapley_f32(x, b[:99], [0, 4], [2, 1], o), "baseline holds 99 values"),
    (lambda e, x, b, o: e.shapley_f32(x, b, list(range(13)), [1] * 13, o), "13 spans"),
    (lambda e, x, b, o: e.shapley_f32(x, b, [], [], o), "0 spans"),
    (lambda e, x, b, o: e.shapley_f32(x, b, [0, 4], [2, 1], o.float()), "phi must be a contiguous fp64"),
    (lambda e, x, b, o: e.shapley_f32(x, b, [0, 4], [2, 1], o, 1), "outside phi's 64"),
    (lambda e, x, b, o: e.shapley_f32(x, b, [0, 1], [2, 1], o), "launcher refused: a span is empty, outside"),  # overlap
    (lambda e, x, b, o: e.shapley_f32(x, b, [4, 0], [1, 2], o), "launcher refused: a span"),  # out of source order
    (lambda e, x, b, o: e.shapley_f32(x, b, [0, 99], [2, 2], o), "launcher refused: a span"),  # past F
    (lambda e, x, b, o: e.shapley_f32(x, b, [0, 4], [2, 0], o), "launcher refused: a span"),  # empty
    (lambda e, x, b, o: _direct(e, x, b, o, scratch=torch.empty(1000, device=DEV)), "the scratch buffer is too small"),
    (lambda e, x, b, o: _direct(e, x, b, o, coef=torch.zeros(2, 2, dtype=torch.float64)), r"coef must be .* \[2\]\[3\]"),
    (lambda e, x, b, o: _direct(e, x, b, o, off=torch.tensor([0, 4], dtype=torch.int32, device=DEV)), "int32 CPU vectors"),
    (lambda e, x, b, o: _direct(e, x, b, o, p_out=torch.empty(3, 64, device=DEV)), r"p_out must be .* \[4\]"),
])
def test_refusals(call, msg):
    eng = _engine(100, torch.zeros(MlpLayout(100, HID).numel))
    ((W1, b1), (W2, b2)), w3, b3 = eng.lay.views(eng.params)
    eng._views = lambda: (W1, b1, W2, b2, w3, b3)
    x, phi = torch.zeros(64, 102, device=DEV), torch.full((2, 64), NAN, dtype=torch.float64, device=DEV)
    eng.pred.fill_(NAN)
    with pytest.raises((RuntimeError, ValueError), match=msg):
        call(eng, x, torch.zeros(100, device=DEV), phi)
    torch.cuda.synchronize()
    assert eng.pred.isnan().all() and phi.isnan().all()


def test_exact_job_on_the_device(tmp_path):
    """The job through the kernel against the oracle route. Both forwards are fp32 sums of no more terms than
    ep(S) counts, so per row |phi_c - oracle| <= y_std * sum over the 2^K coalitions of |w| * 2 ep(S).
    A column the model cannot read: p(S + c) = p(S) exactly, and the rule adds -p w, +p w in ascending i. For
    picked column 0 the two are neighbours, so every pair cancels from 0.0 and phi is exactly 0.0. For column
    c > 0, 2^c other terms stand between them and fp64 rounds the partial sums. The 2^K terms of a column have
    |w| summing to 2, so the products and the adds round by at most 2^(K + 2) 2^-53 max |p|: phi_glr is zero
    to that, not to the bit (the measured figure is in profiles/r12/mlp_f32_shap/README.md)."""
    from wellflow.data.features import FeaturePipeline
    from wellflow.data.io import load_table, write_csv
    from wellflow.data.schema import parse_schema
    from wellflow.explain import run_explain
    from wellflow.models import registry
    from wellflow.predict import Predictor
    from wellflow.utils.checkpoint import save_mdl

    schema = parse_schema(NAMES, TYPES)
    table = load_table("synth", schema, synth_wells=8, synth_steps=100, seed=3)
    pipe = FeaturePipeline(schema, "flow", standardize_target=True).fit(table)
    torch.manual_seed(0)
    ref = MLPRegressor(pipe.n_features, HID)
    glr = pipe.n_features - len(pipe.continuous) + list(pipe.continuous).index("glr")
    off, size = pipe.block_spec()
    with torch.no_grad():  # the model reads neither glr nor the first input column
        next(ref.parameters())[:, glr] = 0.0
        next(ref.parameters())[:, off[0] : off[0] + size[0]] = 0.0
    mdl = str(tmp_path / "models" / "mlp.mdl")
    save_mdl(mdl, "mlp", registry.keras_layers("mlp", ref), {"features": pipe.state()})
    path = str(tmp_path / "data.csv")
    write_csv(table, path, columns=NAMES.split(","))
    table = load_table(path, schema)  # what the job reads

    res = run_explain("mlp", [NAMES, TYPES, "flow", str(tmp_path) + "/", path, "--method", "exact", "--batch-size", "256"],
                      log=lambda *a, **k: None)
    cols, K, n = res["columns"], len(res["columns"]), 800
    assert res["native"] and K == 9 and res["phi"].shape == (K, n) and res["out"].endswith("explain/mlp.csv")
    pmax = np.abs(res["prediction"]).max()
    assert np.abs(res["residual"]).max() <= 1e-9 * pmax
    ora = ExactShapley(Predictor.load(mdl, schema, device="cuda", precision="fp32"), note=lambda s: None).run(table)
    assert not ora["native"] and ora["columns"] == cols

    job = ExactShapley(Predictor.load(mdl, schema, device="cuda", precision="fp32-native", batch=256), piece_rows=512)
    out = job.run(table)  # two pieces, chunks of 256 rows: the same figures
    assert np.array_equal(out["phi"], res["phi"]) and np.array_equal(out["base"], res["base"])
    so, sz = job.ig.spans()
    p64, ep = _coalitions64(job.pred.eng.params.cpu(), torch.from_numpy(pipe.features(table)),
                            torch.from_numpy(job.ig.baseline_row(table, n)), list(zip(so.tolist(), sz.tolist())))
    round64 = 2.0 ** (K + 2 - 53) * float(p64.abs().max()) * pipe.y_std  # of one route's rule
    w_in, w_out = shapley_weights(K)
    pop = np.asarray([bin(i).count("1") for i in range(1 << K)])
    bound = np.stack([(np.where((np.arange(1 << K) >> c) & 1, w_in[pop], w_out[pop])[:, None] * 2 * ep.numpy()).sum(0)
                      for c in range(K)]) * pipe.y_std + 2 * round64
    diff = np.abs(out["phi"] - ora["phi"])
    rel = (diff / np.maximum(np.abs(ora["phi"]), 1e-300))[np.abs(ora["phi"]) > round64]  # not the unread columns
    zero = np.abs(out["phi"][cols.index("glr")]).max()
    print(f"max |residual| {np.abs(res['residual']).max():.3e}; kernel vs oracle route, relative phi difference: median "
          f"{np.median(rel):.3e}, max {rel.max():.3e}; worst difference/bound {(diff / bound).max():.2e}; "
          f"max |phi_glr| {zero:.3e}")
    assert (diff <= bound).all()
    assert (out["phi"][0] == 0.0).all() and np.abs(out["phi"][cols.index("whp")]).max() > 0
    assert zero <= round64
