#!/usr/bin/env python
"""Scoring throughput: device feature assembly (csrc/features.hip) against host assembly.

One process, interleaved timing windows (device / host / device / host ...), so both variants see
the same machine state:

* MLP (hidden 256 x 256) on an in-memory synthetic table of N = 2,097,152 rows and the LSTM
  (H = 512, T = 64) at its full-grid batch: rows/s of ``Predictor.predict_table`` (label codes +
  raw-column upload + assemble_features + forward) against host assembly — ``pipe.features`` (numpy
  one-hot + concatenate + standardise) + the widened upload + the same forward, the only way to
  build engine input before the device kernel existed. Each path is also split into its host
  stage (label lookup / feature matrix) and its device stage (upload + kernels), because the
  per-value label lookup of the host path dominates its total.
* the assembly kernel alone: achieved GB/s (bytes read + written, from the shapes) next to a
  device-to-device copy moving the same byte count.
* ``--wide-forward`` (instead of the above): ``NativeMLP.forward`` over N resident bf16 rows at
  Fp = 72, 128, 256, 512, the fused wide kernel (csrc/mlp_wide.hip) against the per-layer route.

    python tools/predict_throughput.py [--rows N] [--rounds R] [--json PATH] [--wide-forward]
"""
from __future__ import annotations

import argparse
import contextlib
import json
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from wellflow.data.features import FeaturePipeline, take  # noqa: E402
from wellflow.data.io import load_table  # noqa: E402
from wellflow.data.schema import parse_schema  # noqa: E402
from wellflow.ops import native  # noqa: E402

from throughput_common import _clock, _events, _median, _predictor  # noqa: E402

NAMES = "well,field,t,whp,choke,glr,temp,water_cut,dsp,flow"
TYPES = "string,string,int,float,float,float,float,float,float,float"


@contextlib.contextmanager
def host_assembly():
    """``Predictor.predict_table`` on its host-assembly route (that of tables wider than the device
    assembly takes): the feature matrix built by numpy and uploaded, then the same forward."""
    keep, native.ASSEMBLE_MAX_F = native.ASSEMBLE_MAX_F, 0
    try:
        yield
    finally:
        native.ASSEMBLE_MAX_F = keep


def mlp_score(pred, table, stages, host_stage):
    """One ``predict_table``; ``host_stage`` (the label lookup / the feature matrix) is timed alone
    first, because predict_table redoes it."""
    t, _ = _clock(lambda: host_stage(table))
    stages["host_stage_s"].append(t)
    t, y = _clock(lambda: pred.predict_table(table))
    stages["device_stage_s"].append(max(t - stages["host_stage_s"][-1], 0.0))
    stages["total_s"].append(t)
    return y


def bench_mlp(rows, rounds, tmp):
    from wellflow.models.mlp import MLPRegressor

    schema = parse_schema(NAMES, TYPES)
    wells = 16
    table = load_table("synth", schema, synth_wells=wells, synth_steps=rows // wells, seed=1)
    n = len(table["flow"])
    pipe = FeaturePipeline(schema, "flow", standardize_target=True).fit(take(table, np.arange(0, n, 32)))
    torch.manual_seed(0)
    pred = _predictor(tmp, "mlp", MLPRegressor(pipe.n_features, (256, 256)), pipe, schema)
    dev = {"host_stage_s": [], "device_stage_s": [], "total_s": []}
    host = {"host_stage_s": [], "device_stage_s": [], "total_s": []}
    yd = mlp_score(pred, table, {k: [] for k in dev}, pipe.raw_columns)  # warm-up of both paths (engine, code objects)
    with host_assembly():
        yh = mlp_score(pred, table, {k: [] for k in host}, pipe.features)
    same = bool(np.array_equal(yd, yh))
    for _ in range(rounds):
        mlp_score(pred, table, dev, pipe.raw_columns)
        with host_assembly():
            mlp_score(pred, table, host, pipe.features)
    rec = {"rows": n, "features": pipe.n_features, "engine_batch": pred.eng_batch, "bit_identical": same}
    for name, st in (("device_assembly", dev), ("host_assembly", host)):
        rec[name] = {k: _median(v) for k, v in st.items()}
        rec[name]["rows_per_s"] = n / rec[name]["total_s"]
        rec[name]["rows_per_s_device_stage"] = n / rec[name]["device_stage_s"]
        rec[name]["all_total_s"] = [round(v, 4) for v in st["total_s"]]
    return rec, (pipe, table)


def bench_lstm(rounds, tmp):
    from wellflow.models.lstm import LSTMRegressor, NativeLSTM

    H, T, wells = 512, 64, 8
    dev = torch.device("cuda", 0)
    B = NativeLSTM.full_grid_batch(H, dev)
    schema = parse_schema(NAMES, TYPES)
    table = load_table("synth", schema, synth_wells=wells, synth_steps=T - 1 + B, seed=2)  # 8 full chunks
    n = len(table["flow"])
    pipe = FeaturePipeline(schema, "flow", standardize_target=True).fit(take(table, np.arange(0, n, 8)))
    torch.manual_seed(0)
    pred = _predictor(tmp, "lstm", LSTMRegressor(pipe.n_features, H), pipe, schema,
                      job={"seq_len": T, "group_col": "well", "hidden": H, "mlp_hidden": [256, 256]}, batch=B)

    def host_score():
        with host_assembly():
            return pred.predict_table(table)

    yd = pred.predict_table(table)
    yh = host_score()
    td, th = [], []
    for _ in range(rounds):
        td.append(_clock(lambda: pred.predict_table(table))[0])
        th.append(_clock(host_score)[0])
    windows = int((~np.isnan(yd)).sum())
    pred.eng.check_device_errors()
    return {"rows": n, "windows": windows, "engine_batch": B, "features": pipe.n_features,
            "bit_identical": bool(np.array_equal(yd, yh, equal_nan=True)),
            "device_assembly": {"total_s": _median(td), "windows_per_s": windows / _median(td), "all_total_s": td},
            "host_assembly": {"total_s": _median(th), "windows_per_s": windows / _median(th), "all_total_s": th}}


def bench_kernel(pipe, table, rounds, launches=20):
    """assemble_features alone (resident raw columns) vs a D2D copy of the same byte count."""
    dev = torch.device("cuda", 0)
    codes, cont = pipe.raw_columns(table)
    off, size = pipe.block_spec()
    mean, std = pipe.scale()
    codes_d, cont_d = torch.from_numpy(codes).to(dev), torch.from_numpy(cont).to(dev)
    spec = [torch.from_numpy(np.ascontiguousarray(v)).to(dev) for v in (off, size, mean, std)]
    C = native.lib()
    n, F = codes.shape[1], pipe.n_features
    out = {}
    for label, dt in (("bf16", torch.bfloat16), ("fp32", torch.float32)):
        ld = (F + 7) // 8 * 8 if dt == torch.bfloat16 else F
        nbytes = codes.nbytes + cont.nbytes + n * ld * (2 if dt == torch.bfloat16 else 4)
        dst = torch.empty((n, ld), dtype=dt, device=dev)
        a = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)  # a copy reads and writes: same total bytes
        b = torch.empty_like(a)
        run_k = lambda: C.assemble_features(codes_d, cont_d, *spec, 0, n, F, dst, -1, None)  # noqa: E731  (the launch alone)
        run_c = lambda: b.copy_(a)  # noqa: E731
        tk, tc = [], []
        for fn in (run_k, run_c):
            fn()
        for _ in range(rounds):
            for fn, acc in ((run_k, tk), (run_c, tc)):
                acc.append(_events(fn, launches))
        out[label] = {"rows": n, "ld": ld, "bytes": nbytes, "kernel_us": _median(tk) * 1e6,
                      "kernel_GBps": nbytes / _median(tk) / 1e9, "copy_us": _median(tc) * 1e6,
                      "copy_GBps": nbytes / _median(tc) / 1e9}
    return out


def bench_wide_forward(rows, rounds, widths=(72, 128, 256, 512), launches=5):
    """``NativeMLP.forward`` over ``rows`` resident bf16 rows at Fp > 64: the fused wide kernel
    (csrc/mlp_wide.hip) against the per-layer route (``wide_fwd=False``: two GEMMs + head_fwd) on
    the same engine, windows interleaved; X bytes/s = rows * Fp * 2 over the call time."""
    from wellflow.models.mlp import NativeMLP, init_mlp_flat

    dev = torch.device("cuda", 0)
    out = {}
    for F in widths:
        eng = NativeMLP(F, (256, 256), rows, device=dev, params=init_mlp_flat(F).to(dev))
        X = eng.to_input_format(torch.randn(rows, F, device=dev))
        t = {True: [], False: []}
        pred = {}
        for wide in (True, False):  # warm-up, and the outputs to compare
            eng.wide_fwd = wide
            pred[wide] = eng.forward(X).clone()
        for _ in range(rounds):
            for wide in (True, False):
                eng.wide_fwd = wide
                t[wide].append(_events(lambda: eng.forward(X), launches))
        tw, tp = _median(t[True]), _median(t[False])
        out[f"Fp{eng.Fp}"] = {"rows": rows, "Fp": eng.Fp, "wide_ms": tw * 1e3, "per_layer_ms": tp * 1e3,
                              "per_layer_over_wide": tp / tw, "wide_x_GBps": rows * eng.Fp * 2 / tw / 1e9,
                              "per_layer_x_GBps": rows * eng.Fp * 2 / tp / 1e9,
                              "wide_rows_per_s": rows / tw, "per_layer_rows_per_s": rows / tp,
                              "max_abs_diff": (pred[True] - pred[False]).abs().max().item(),
                              "pred_abs_max": pred[False].abs().max().item(),
                              "all_wide_ms": [round(v * 1e3, 4) for v in t[True]],
                              "all_per_layer_ms": [round(v * 1e3, 4) for v in t[False]]}
        del eng, X, pred
        torch.cuda.empty_cache()
    return out


def _spread(v, scale=1e3):
    return {"median": _median(v) * scale, "min": min(v) * scale, "max": max(v) * scale}


def bench_f32(rows, rounds, tmp, widths=(16, 72, 128, 512)):
    """One scoring pass (``MlpPass.score()``, resident raw columns: assembly + forward) over ``rows``
    in-memory rows on three routes, windows interleaved: ``bf16`` (device assembly + the bf16 fused
    forwards), ``fp32-native`` (fp32 device assembly + csrc/mlp_f32.hip) and ``fp32`` (the PyTorch
    oracle: host assembly, upload, torch). Then the forward alone over the same device-assembled
    fp32 rows: ``NativeMLP.forward_f32`` against torch's fp32 forward of the same weights on the
    device. Times in ms: median, min, max over the rounds."""
    from wellflow.models.mlp import MLPRegressor
    from wellflow.scoring import MlpPass

    out = {}
    for Fp in widths:
        L, Q = Fp - 8, 8  # one categorical column of L labels + 8 continuous ones: F = Fp
        rng = np.random.default_rng(Fp)
        names = ["c0"] + [f"x{i}" for i in range(Q)] + ["y"]
        schema = parse_schema(",".join(names), ",".join(["string"] + ["float"] * (Q + 1)))
        pool = np.asarray([f"l{k:03d}" for k in range(L)], dtype=object)
        table = {"c0": pool[rng.integers(0, L, rows)]}
        for c in names[1:]:
            table[c] = rng.normal(size=rows).astype(np.float32)
        pipe = FeaturePipeline(schema, "y", standardize_target=True).fit(take(table, np.arange(0, rows, 16)))
        torch.manual_seed(0)
        ref = MLPRegressor(pipe.n_features, (256, 256))
        routes = ("bf16", "fp32-native", "fp32")
        ps = {r: MlpPass(_predictor(tmp, "mlp", ref, pipe, schema, precision=r), table, resident=True) for r in routes}
        with torch.no_grad():
            y = {r: torch.as_tensor(ps[r].score()).float().cpu().clone() for r in routes}  # warm-up, and the outputs
            t = {r: [] for r in routes}
            for _ in range(rounds):
                for r in routes:
                    t[r].append(_clock(ps[r].score)[0])
            # the forward alone, over the fp32 rows the device assembly wrote
            pn = ps["fp32-native"]
            X = pn.assemble(*pn.pieces[0])
            net = ref.to(X.device)
            fwd = {"fp32-native": lambda: pn.forward(X, 0), "torch_fp32": lambda: net(X)}
            ydev = net(X).cpu()
            tk = {k: [] for k in fwd}
            for _ in range(rounds):
                for k, fn in fwd.items():
                    tk[k].append(_events(fn, 3))
        rec = {"rows": rows, "features": pipe.n_features, "engine_batch": ps["bf16"].B,
               "pass_ms": {r: _spread(t[r]) for r in routes}, "forward_ms": {k: _spread(v) for k, v in tk.items()},
               "fp32_over_fp32_native_pass": _median(t["fp32"]) / _median(t["fp32-native"]),
               "torch_over_kernel_forward": _median(tk["torch_fp32"]) / _median(tk["fp32-native"]),
               "max_abs_diff_vs_fp32": {r: (y[r] - y["fp32"]).abs().max().item() for r in routes[:2]},
               "max_abs_diff_kernel_vs_torch_on_device": (y["fp32-native"][: len(ydev)] - ydev).abs().max().item(),
               "pred_abs_max": y["fp32"].abs().max().item()}
        out[f"Fp{Fp}"] = rec
        print(json.dumps({f"Fp{Fp}": rec}), flush=True)
        del ps, X, net, table, y
        torch.cuda.empty_cache()
    return out


def f32_job_accuracy(tmp):
    """What of the bf16 route's documented distance to the fp32 oracle is left in ``fp32-native``, on
    the fitted MLP of the set-point and interval job tests (18 -> 256 -> 256 -> 1, 200 Adam steps on
    8 wells x 125 rows): set-point statuses of 1000 rows that differ, and the worst relative
    difference of the 27 calibration quantiles (3 levels x 8 wells + overall)."""
    from wellflow.interval import ConformalBands
    from wellflow.models.mlp import MLPRegressor
    from wellflow.predict import Predictor
    from wellflow.setpoint import SetPoint

    schema = parse_schema(NAMES, TYPES)
    table = load_table("synth", schema, synth_wells=8, synth_steps=125, seed=3)
    pipe = FeaturePipeline(schema, "flow", standardize_target=True).fit(table)
    torch.manual_seed(0)
    ref = MLPRegressor(pipe.n_features, (256, 256))
    X = torch.from_numpy(pipe.features(table))
    y = torch.from_numpy(np.asarray(pipe.target_values(table), np.float32)).reshape(-1)
    opt = torch.optim.Adam(ref.parameters(), lr=2e-3)
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        for _ in range(200):
            opt.zero_grad()
            ((ref(X).reshape(-1) - y) ** 2).mean().backward()
            opt.step()
    finally:
        torch.set_num_threads(threads)
    _predictor(tmp, "mlp", ref, pipe, schema)  # saves <tmp>/models/mlp.mdl
    path = os.path.join(tmp, "models", "mlp.mdl")
    want, alphas = np.asarray(table["flow"], np.float32), ("0.1", "0.05", "0.5")

    def run(device, precision):
        sp = SetPoint(Predictor.load(path, schema, device=device, precision=precision, batch=512), points=9,
                      refine=6).run(table, "choke", want)
        cb = ConformalBands(Predictor.load(path, schema, device=device, precision=precision, batch=512), alphas=alphas,
                            by="well").calibrate(table)
        return sp["bracket"], np.asarray([r["quantile"] for r in cb["rows"]])

    b0, q0 = run("cpu", "fp32")
    out = {}
    for precision in ("bf16", "fp32-native"):
        b, q = run("cuda", precision)
        rel = np.abs(q - q0) / q0
        out[precision] = {"setpoint_status_differs_of_1000": int((np.asarray(b) != np.asarray(b0)).sum()),
                          "quantiles": len(rel), "quantile_rel_max": float(rel.max()),
                          "quantile_rel_median": float(np.median(rel))}
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=2_097_152)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--json", default="")
    ap.add_argument("--skip-lstm", action="store_true")
    ap.add_argument("--wide-forward", action="store_true",
                    help="only the MLP forward at Fp = 72, 128, 256, 512: fused wide kernel vs per-layer route")
    ap.add_argument("--f32", action="store_true",
                    help="only one scoring pass at Fp = 16, 72, 128, 512 on three routes: bf16, fp32-native (the fp32 "
                         "kernel) and fp32 (the PyTorch oracle); and the fp32 kernel alone against torch on the device")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("predict_throughput: needs a GPU (no rate is reported without one)", file=sys.stderr)
        return 2
    rec = {"device": torch.cuda.get_device_name(0)}
    with tempfile.TemporaryDirectory() as tmp:
        if args.f32:
            rec["mlp_f32_jobs_vs_fp32_oracle"] = f32_job_accuracy(tmp)
            print(json.dumps(rec), flush=True)
            rec["mlp_f32"] = bench_f32(args.rows, args.rounds, tmp)
        elif args.wide_forward:
            rec["mlp_wide_forward"] = bench_wide_forward(args.rows, args.rounds)
        else:
            rec["mlp"], (pipe, table) = bench_mlp(args.rows, args.rounds, tmp)
            rec["assemble_kernel"] = bench_kernel(pipe, table, max(args.rounds, 5))
            del table
            if not args.skip_lstm:
                rec["lstm"] = bench_lstm(args.rounds, tmp)
    line = json.dumps(rec)
    print(line)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
