"""Prediction on the GPU: the device feature-assembly kernel (csrc/features.hip) against the host
pipeline bit for bit, and the native scoring paths of wellflow/predict.py."""
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


def _rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return ((a - b).norm() / b.norm()).item()


# ------------------------------------------------------------------ 1. the assembly kernel
N_MAX = 70001
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
    """(pipe, table, X fp32 [N_MAX][F]) of a column set: the host pipeline's output, computed once."""
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
    fit_rows = np.flatnonzero(seen)[:20000]
    pipe = FeaturePipeline(schema, "y").fit(take(table, fit_rows))
    assert [len(ix.labels) for ix in pipe.indexers] == list(labels) and pipe.n_features == sum(labels) + Q
    X = pipe.transform(table)[0]
    _REF[key] = (pipe, table, X)
    return _REF[key]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("key", list(COLUMN_SETS))
def test_assemble_features_equals_host_pipeline(key, n):
    from wellflow.models.mlp import NativeMLP
    from wellflow.ops.native import assemble_features

    pipe, table, X = _reference(key)
    sub = take(table, np.arange(n))
    codes, cont = pipe.raw_columns(sub)
    off, size = pipe.block_spec()
    mean, std = pipe.scale()
    F = pipe.n_features
    Fp = (F + 7) // 8 * 8
    if codes.shape[0]:
        assert codes.max() <= max(len(ix.labels) for ix in pipe.indexers)
    want32 = torch.from_numpy(X[:n])
    # fp32 row table (the LSTM's): [N][F]
    out32 = torch.full((n, F), float("nan"), device=DEV)
    got = assemble_features(codes, cont, off, size, mean, std, F, torch.float32, DEV, out=out32)
    torch.cuda.synchronize()
    assert got.data_ptr() == out32.data_ptr() and torch.equal(out32.cpu(), want32)
    # bf16 MLP input format: [N][Fp], padding written as zeros (the buffer starts as NaN)
    stub = types.SimpleNamespace(F=F, Fp=Fp)
    want16 = NativeMLP.to_input_format(stub, want32)
    out16 = torch.full((n, Fp), float("nan"), dtype=torch.bfloat16, device=DEV)
    assemble_features(codes, cont, off, size, mean, std, F, torch.bfloat16, DEV, out=out16)
    torch.cuda.synchronize()
    assert want16.shape == (n, Fp) and torch.equal(out16.cpu().view(torch.int16), want16.view(torch.int16))
    if key == "c3_17_q7" and n == N_MAX:
        assert (codes[1] == 17).any() and (codes[0] == 3).any()  # unseen labels were in the rows


def test_assemble_features_widest_table_and_refusals():
    """F = 512 is the widest the binding takes (a 131-KB fp32 tile, one workgroup per CU); a
    block spec that does not tile the row is refused on the host before anything is launched."""
    from wellflow.ops.native import assemble_features

    rng = np.random.default_rng(7)
    n, Q = 130, 512
    cont = rng.normal(size=(Q, n)).astype(np.float32) * 50
    mean, std = rng.normal(size=Q).astype(np.float32), rng.uniform(0.5, 2.0, size=Q).astype(np.float32)
    want = ((cont - mean[:, None]) / std[:, None]).T.copy()
    none = np.zeros((0, n), np.int32)
    out = torch.full((n, Q), float("nan"), device=DEV)
    assemble_features(none, cont, [], [], mean, std, Q, torch.float32, DEV, out=out)
    assert torch.equal(out.cpu(), torch.from_numpy(want))
    out16 = assemble_features(none, cont, [], [], mean, std, Q, torch.bfloat16, DEV)
    assert torch.equal(out16.cpu().view(torch.int16), torch.from_numpy(want).to(torch.bfloat16).view(torch.int16))
    with pytest.raises(RuntimeError, match="512"):
        big = np.zeros((513, 4), np.float32)
        assemble_features(np.zeros((0, 4), np.int32), big, [], [], np.zeros(513, np.float32), np.ones(513, np.float32),
                          513, torch.float32, DEV)
    codes = np.zeros((1, n), np.int32)
    with pytest.raises(ValueError, match="back to back"):
        assemble_features(codes, cont[:2], [3], [4], mean[:2], std[:2], 6, torch.float32, DEV)
    with pytest.raises(ValueError, match="F = 9"):
        assemble_features(codes, cont[:2], [0], [4], mean[:2], std[:2], 9, torch.float32, DEV)
    # an empty table: an empty result of the asked dtype and width, nothing launched
    for dt, ld in ((torch.float32, 6), (torch.bfloat16, 8)):
        empty = assemble_features(codes[:, :0], cont[:2, :0], [0], [4], mean[:2], std[:2], 6, dt, DEV)
        assert empty.shape == (0, ld) and empty.dtype == dt and empty.device == DEV


# ------------------------------------------------------------------ 2. MLP scoring
def _mlp_case(tmp_path):
    """1000 rows, F = 18, a saved 18-256-256-1 MLP: (schema, table, pipe, ref, .mdl path)."""
    from wellflow.models.mlp import MLPRegressor

    schema = parse_schema(NAMES, TYPES)
    table = load_table("synth", schema, synth_wells=8, synth_steps=125, seed=3)
    pipe = FeaturePipeline(schema, "flow", standardize_target=True).fit(table)
    assert pipe.n_features == 18  # 8 well columns + 3 field columns + 7 continuous
    torch.manual_seed(0)
    ref = MLPRegressor(18, (256, 256))
    p = str(tmp_path / "models" / "mlp.mdl")
    save_mdl(p, "mlp", registry.keras_layers("mlp", ref), {"features": pipe.state()})
    return schema, table, pipe, ref, p


def test_native_mlp_scoring_two_chunks(tmp_path):
    from wellflow.predict import Predictor

    schema, table, pipe, ref, p = _mlp_case(tmp_path)
    pred = Predictor.load(p, schema, device="cuda", precision="bf16", batch=512)
    got = pred.predict_table(table)  # 1000 rows: a full chunk of 512 and a short one of 488
    assert pred.native and pred.eng_batch == 512 and got.shape == (1000,) and got.dtype == np.float32
    eng = pred.eng
    Xh = eng.to_input_format(torch.from_numpy(pipe.transform(table)[0])).to(DEV)
    host = torch.cat([eng.forward(Xh[a : a + 512]).clone() for a in (0, 512)]).cpu().numpy()
    assert np.array_equal(got, np.asarray(pipe.inverse_target(host), np.float32))
    with torch.no_grad():
        want = ref(torch.from_numpy(pipe.transform(table)[0])).numpy()
    rel = _rel((got.astype(np.float64) - pipe.y_mean) / pipe.y_std, want)
    print("mlp scoring rel-L2 vs fp32:", rel)
    assert rel < 2e-2, rel
    assert _rel(got, pipe.inverse_target(want)) < 2e-2


def test_native_mlp_scoring_in_pieces(tmp_path):
    """piece_rows = 512: two pieces, each with its own raw-column upload and assembly, the second
    a short chunk of 488 rows. The same launches on the same rows as the one-piece run."""
    from wellflow.predict import Predictor

    schema, table, pipe, ref, p = _mlp_case(tmp_path)
    pred = Predictor.load(p, schema, device="cuda", precision="bf16", batch=512)
    whole = pred.predict_table(table)
    pred.piece_rows = 512
    pieced = pred.predict_table(table)
    assert pred.native and pred.eng_batch == 512 and pieced.shape == (1000,) and np.isfinite(pieced).all()
    assert np.array_equal(pieced, whole)


def test_native_mlp_host_assembly_equals_device_assembly(tmp_path, monkeypatch):
    """Above the device assembly's width limit the rows are built on the host and uploaded; the
    native engine then gives the same predictions bit for bit."""
    from wellflow.predict import Predictor

    schema, table, pipe, ref, p = _mlp_case(tmp_path)
    pred = Predictor.load(p, schema, device="cuda", precision="bf16", batch=512)
    dev = pred.predict_table(table)
    monkeypatch.setattr("wellflow.ops.native.ASSEMBLE_MAX_F", 8)
    host = pred.predict_table(table)
    assert pred.native and dev.shape == (1000,) and np.isfinite(dev).all()
    assert np.array_equal(host, dev)


# ------------------------------------------------------------------ 3. LSTM scoring
def _lstm_case(tmp_path):
    """150 rows in 3 interleaved series, T = 8, F = 16, a saved H = 128 LSTM."""
    from wellflow.models.lstm import LSTMRegressor

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
    return schema, table, pipe, ref, p, (T, H, n)


def test_native_lstm_scoring_padded_last_chunk(tmp_path):
    from wellflow.predict import Predictor

    schema, table, pipe, ref, p, (T, H, n) = _lstm_case(tmp_path)
    pred = Predictor.load(p, schema, device="cuda", precision="bf16", batch=64)
    got = pred.predict_table(table)
    eng = pred.eng
    assert pred.native and pred.eng_batch == 64 and eng.H == H and eng.T == T
    nan = np.isnan(got)
    assert nan.sum() == 21 and np.array_equal(np.flatnonzero(nan), np.arange(21))
    # the same windows, gathered on the host and run through the engine's ordinary forward
    ids = np.unique(table["well"].astype(str), return_inverse=True)[1]
    order = np.argsort(ids, kind="stable")
    X = pipe.features(take(table, order))
    starts = window_starts(n, T, ids[order])
    assert len(starts) == 129  # three chunks of 64: the last holds one window + 63 padding ids
    Xw = torch.from_numpy(X[starts[:, None] + np.arange(T)[None, :]]).to(DEV)
    host = torch.cat([eng.forward(Xw[a : a + 64]).clone() for a in range(0, 129, 64)]).cpu().numpy()
    want_rows = order[starts + T - 1]
    assert np.array_equal(got[want_rows], host)
    assert np.array_equal(np.sort(want_rows), np.flatnonzero(~nan))
    with torch.no_grad():
        fp32 = ref(Xw.cpu()).numpy()
    err = np.abs(got[want_rows] - fp32).max()
    print("lstm scoring max abs err vs fp32:", err)
    assert err < 3e-2, err
    assert eng.persistent_error() == 0, eng.persistent_stats()


def test_native_lstm_host_assembly_equals_device_assembly(tmp_path, monkeypatch):
    """129 windows in batches of 64 (the last chunk: one window + padding), the row table built on
    the host and uploaded: bit-identical to the device-assembled one, NaN in the same rows."""
    from wellflow.predict import Predictor

    schema, table, pipe, ref, p, (T, H, n) = _lstm_case(tmp_path)
    pred = Predictor.load(p, schema, device="cuda", precision="bf16", batch=64)
    dev = pred.predict_table(table)
    monkeypatch.setattr("wellflow.ops.native.ASSEMBLE_MAX_F", 8)
    host = pred.predict_table(table)
    assert pred.native and pred.eng_batch == 64 and (~np.isnan(dev)).sum() == 129
    assert np.array_equal(host, dev, equal_nan=True)
    assert pred.eng.persistent_error() == 0, pred.eng.persistent_stats()


# ------------------------------------------------------------------ 4. CNN scoring
def test_native_cnn_scoring_reference_shape(tmp_path):
    from wellflow.models.cnn import CNN1DRegressor
    from wellflow.predict import Predictor

    schema = parse_schema(NAMES, TYPES)
    table = load_table("synth", schema, synth_wells=2, synth_steps=100, seed=5)
    pipe = FeaturePipeline(schema, "flow", standardize_target=True).fit(table)
    ref = CNN1DRegressor().init_keras(2)
    p = str(tmp_path / "models" / "cnn.mdl")
    save_mdl(p, "cnn", registry.keras_layers("cnn", ref), {"features": pipe.state()})
    pred = Predictor.load(p, schema, device="cuda", precision="bf16")
    end_rows, fc = pred.predict_table(table)
    assert pred.native and fc.shape == (106, 12)
    assert np.array_equal(end_rows, np.concatenate([np.arange(47, 100), np.arange(147, 200)]))
    y = pipe.target_values(table)
    ref.eval()
    with torch.no_grad():
        want = ref(torch.from_numpy(np.stack([y[e - 47 : e + 1] for e in end_rows]))[:, :, None]).numpy()
    rel = _rel((fc.astype(np.float64) - pipe.y_mean) / pipe.y_std, want)
    print("cnn scoring rel-L2 vs fp32:", rel)
    assert rel < 2e-2, rel


# ------------------------------------------------------------------ 5. end to end
def test_train_then_predict_job_on_the_gpu(tmp_path):
    from wellflow.predict import run_predict
    from wellflow.train.job import run_job

    sp = str(tmp_path) + "/"
    out = run_job("mlp", [NAMES, TYPES, "flow", sp, "--max-steps", "20", "--synth-wells", "4", "--synth-steps", "200",
                          "--verbose", "0"], **QUIET)
    assert out["native"]
    schema = parse_schema(NAMES, TYPES)
    table = load_table("synth", schema, synth_wells=4, synth_steps=200, seed=42)
    path = str(tmp_path / "data.csv")
    write_csv(table, path, columns=NAMES.split(","))
    a = run_predict("mlp", [NAMES, TYPES, "flow", sp, path], **QUIET)
    b = run_predict("mlp", [NAMES, TYPES, "flow", sp, path, "--precision", "fp32", "--out", str(tmp_path / "fp32.csv")],
                    **QUIET)
    assert a["native"] and not b["native"]
    for r in (a, b):
        with open(r["out"], newline="") as f:
            rows = list(csv.reader(f))
        assert len(rows) == 800 and all(len(x) == 11 and x[-1] != "" for x in rows)
        assert np.allclose(np.asarray([float(x[-1]) for x in rows]), r["predictions"], rtol=1e-6)
    rel = _rel(a["predictions"], b["predictions"])
    print("job predictions, native vs fp32, rel-L2:", rel)
    assert rel < 2e-2, rel
    assert a["mse"] is not None and b["mse"] is not None
