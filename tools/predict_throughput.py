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

    python tools/predict_throughput.py [--rows N] [--rounds R] [--json PATH]
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


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=2_097_152)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--json", default="")
    ap.add_argument("--skip-lstm", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("predict_throughput: needs a GPU (no rate is reported without one)", file=sys.stderr)
        return 2
    rec = {"device": torch.cuda.get_device_name(0)}
    with tempfile.TemporaryDirectory() as tmp:
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
