#!/usr/bin/env python
"""Permutation-importance throughput: passes/s of the device pass loop (wellflow/importance.py)
against what a user could do before it — permute the column on the host and call
``Predictor.predict_table`` once per pass, then take the error in numpy — on the same commit.

One process, interleaved timing windows (device / host / device / host ...), so both variants see
the same machine state. Two shapes:

* MLP 16-256-256-1 on an in-memory synthetic table of N = 2,097,152 rows (6 wells: 6 + 3 one-hot
  columns + 7 continuous);
* LSTM (H = 512, T = 64) at its full-grid batch, 8 full chunks of windows.

A device window is ``--passes`` passes of the pass loop with ONE synchronisation at its end (the
job's shape: the host reads the sums once); a host window is ``--host-passes`` passes of host
permute + ``predict_table`` + numpy error. The terms of a device pass (randperm, permuted
assembly, forward(s), reduction) are also timed alone with device events, 10 launches per window.

    python tools/importance_throughput.py [--rows N] [--rounds R] [--json PATH]
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o run -- \\
        python tools/importance_throughput.py --profile-run       # the kernels' own times
"""
from __future__ import annotations

import argparse
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
from wellflow.importance import ErrorSums  # noqa: E402
from wellflow.scoring import PermutedColumn  # noqa: E402
from wellflow.whatif import LearnedScorer  # noqa: E402

from throughput_common import _clock, _events, _median, _predictor  # noqa: E402

NAMES = "well,field,t,whp,choke,glr,temp,water_cut,dsp,flow"
TYPES = "string,string,int,float,float,float,float,float,float,float"


def _measure(pred, table, err, cols, passes, host_passes, rounds):
    """Interleaved device / host windows over the columns ``cols`` (source indices), round robin."""
    ps = err.scorer.ps  # the pass (wellflow/scoring.py): its own assembly and forward steps are timed below
    n = len(table["flow"])
    dev = pred.device
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    rng = np.random.default_rng(0)
    y = np.asarray(table["flow"], np.float64)
    names = ps.names
    err.begin(1 + passes)

    def device_window():
        with torch.no_grad():
            for i in range(passes):
                perm = torch.randperm(n, generator=gen, device=dev, dtype=torch.int32)
                err.score(1 + i, PermutedColumn(cols[i % len(cols)], perm))
        return err.finish()  # the one read of the sums

    def host_window():
        out = []
        for i in range(host_passes):
            c = names[cols[i % len(cols)]]
            t2 = dict(table)
            t2[c] = np.asarray(table[c])[rng.permutation(n)]
            p = np.asarray(pred.predict_table(t2), np.float64)
            ok = ~np.isnan(p)
            d = p[ok] - y[ok]
            out.append(float(np.mean(d * d)))
        return out

    with torch.no_grad():
        err.score(0)
    device_window()  # warm-up of both paths
    host_window()
    td, th = [], []
    for _ in range(rounds):
        td.append(_clock(device_window)[0] / passes)
        th.append(_clock(host_window)[0] / host_passes)
    sums = err.finish()
    # the terms of one device pass, each alone
    perm = torch.randperm(n, generator=gen, device=dev, dtype=torch.int32)
    edit = PermutedColumn(cols[0], perm)
    a, b = ps.pieces[0]  # one piece at these sizes
    terms = {"randperm_us": [], "assemble_us": [], "forward_us": [], "reduce_us": []}
    with torch.no_grad():
        for _ in range(max(rounds, 3)):
            terms["randperm_us"].append(_events(lambda: torch.randperm(n, generator=gen, device=dev, dtype=torch.int32)))
            terms["assemble_us"].append(_events(lambda: ps.assemble(a, b, edit)))
            terms["forward_us"].append(_events(lambda: ps.forward(ps.X[: b - a], a)))
            terms["reduce_us"].append(_events(lambda: err.reduce(0)))
    rec = {"device": {"pass_s": _median(td), "passes_per_s": 1.0 / _median(td), "all_pass_s": td, "passes_per_window": passes},
           "host": {"pass_s": _median(th), "passes_per_s": 1.0 / _median(th), "all_pass_s": th,
                    "passes_per_window": host_passes},
           "terms": {k2: _median(v) * 1e6 for k2, v in terms.items()},
           "finite": bool(np.isfinite(sums).all())}
    rec["speedup"] = rec["host"]["pass_s"] / rec["device"]["pass_s"]
    return rec


def bench_mlp(rows, passes, host_passes, rounds, tmp):
    from wellflow.models.mlp import MLPRegressor

    schema = parse_schema(NAMES, TYPES)
    wells = 6  # 6 well + 3 field one-hot columns + 7 continuous = 16 features
    table = load_table("synth", schema, synth_wells=wells, synth_steps=(rows + wells - 1) // wells, seed=1)
    table = take(table, np.arange(rows))  # the last well is a few rows short; every well is still there
    n = len(table["flow"])
    pipe = FeaturePipeline(schema, "flow", standardize_target=True).fit(take(table, np.arange(0, n, 32)))
    torch.manual_seed(0)
    pred = _predictor(tmp, "mlp", MLPRegressor(pipe.n_features, (256, 256)), pipe, schema)
    t_setup, err = _clock(lambda: ErrorSums(LearnedScorer(pred, table, "importance"), np.asarray(table["flow"], np.float64)))
    scorer = err.scorer
    rec = _measure(pred, table, err, list(range(len(scorer.ps.names))), passes, host_passes, rounds)
    rec.update(rows=n, features=pipe.n_features, engine_batch=pred.eng_batch, setup_s=t_setup,
               pieces=len(scorer.ps.pieces))
    return rec


def bench_lstm(passes, host_passes, rounds, tmp):
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
    t_setup, err = _clock(lambda: ErrorSums(LearnedScorer(pred, table, "importance"), np.asarray(table["flow"], np.float64)))
    scorer = err.scorer
    rec = _measure(pred, table, err, list(range(len(scorer.ps.names))), passes, host_passes, rounds)
    pred.eng.check_device_errors()
    rec.update(rows=n, windows=int(scorer.M), features=pipe.n_features, engine_batch=B, setup_s=t_setup)
    return rec


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=2_097_152)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--passes", type=int, default=18, help="device passes per timing window")
    ap.add_argument("--host-passes", type=int, default=2, help="host passes per timing window")
    ap.add_argument("--json", default="")
    ap.add_argument("--skip-lstm", action="store_true")
    ap.add_argument("--profile-run", action="store_true",
                    help="one short round of each shape (for a kernel trace): no rates are worth reading")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("importance_throughput: needs a GPU (no rate is reported without one)", file=sys.stderr)
        return 2
    if args.profile_run:
        args.rounds, args.host_passes = 1, 1
    rec = {"device": torch.cuda.get_device_name(0)}
    with tempfile.TemporaryDirectory() as tmp:
        rec["mlp"] = bench_mlp(args.rows, args.passes, args.host_passes, args.rounds, tmp)
        if not args.skip_lstm:
            rec["lstm"] = bench_lstm(args.passes, args.host_passes, args.rounds, tmp)
    line = json.dumps(rec)
    print(line)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
