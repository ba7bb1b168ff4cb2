#!/usr/bin/env python
"""Response-curve throughput: passes/s of the device pass loop (wellflow/response.py) against what a
user could do without it — replace the column on the host, call ``Predictor.predict_table`` once per
pass, then group the predictions with ``np.bincount`` — on the same commit.

One process, interleaved timing windows (device / host / device / host ...), so both variants see
the same machine state. Two shapes:

* MLP 16-256-256-1 on an in-memory synthetic table of N = 2,097,152 rows (6 wells: 6 + 3 one-hot
  columns + 7 continuous), grouped by well;
* LSTM (H = 512, T = 64) at its full-grid batch, 8 full chunks of windows, grouped by well.

A device window is ``--passes`` passes of the pass loop with ONE synchronisation at its end (the
job's shape: the host reads the sums once); a host window is ``--host-passes`` passes of host
replace + ``predict_table`` + ``np.bincount``. The host-side grouping ALONE (the three bincounts
over M predictions already on the host) is also timed. The terms of a device pass (constant
assembly, forward(s), group_sums) are timed alone with device events, 10 launches per window, and
``group_sums`` against ``err_sums`` on the same M, interleaved, at G = 1 and G = 1,024 (grouped
rows, and at G = 1,024 also scattered ids: the 4-B gather).

    python tools/response_throughput.py [--rows N] [--rounds R] [--json PATH]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from wellflow.data.features import FeaturePipeline, take  # noqa: E402
from wellflow.data.io import load_table  # noqa: E402
from wellflow.data.schema import parse_schema  # noqa: E402
from wellflow.response import GroupSums, group_sums_host  # noqa: E402
from wellflow.scoring import constant  # noqa: E402
from wellflow.whatif import LearnedScorer  # noqa: E402

from throughput_common import _clock, _events, _median, _predictor  # noqa: E402

NAMES = "well,field,t,whp,choke,glr,temp,water_cut,dsp,flow"
TYPES = "string,string,int,float,float,float,float,float,float,float"


def _measure(pred, table, grp, ids, G, passes, host_passes, rounds):
    """Interleaved device / host windows: the continuous column 'choke' swept over ``passes`` values."""
    scorer = grp.scorer
    ps = scorer.ps  # the pass (wellflow/scoring.py): its own assembly and forward steps are timed below
    pipe = pred.pipe
    k = ps.names.index("choke")
    lo, hi = float(np.min(table["choke"])), float(np.max(table["choke"]))
    grid = list(np.linspace(lo, hi, passes, dtype=np.float64).astype(np.float32))
    consts = grp.constants(k, grid, None)  # the one upload of the grid
    grp.begin(1 + passes)

    def device_window():
        with torch.no_grad():
            for i in range(passes):
                grp.score(1 + i, consts[i])
        return grp.finish()  # the one read of the sums

    def host_window():
        out = []
        for i in range(host_passes):
            p = np.asarray(pred.predict_table(constant(table, "choke", grid[i % passes])), np.float64)
            ok = ~np.isnan(p)
            out.append(group_sums_host(p[ok], ids[ok], G))
        return out

    with torch.no_grad():
        grp.score(0)
    dsums = device_window()  # warm-up of both paths
    hsums = host_window()
    # the two paths agree: predict_table rounds the raw-unit prediction to fp32, the device keeps fp64
    rel = float(np.max(np.abs(dsums[1, :, 1] - hsums[0][:, 1]) / np.abs(hsums[0][:, 1])))
    td, th = [], []
    for _ in range(rounds):
        td.append(_clock(device_window)[0] / passes)
        th.append(_clock(host_window)[0] / host_passes)
    sums = grp.finish()
    # the host-side grouping alone: M predictions already on the host -> three bincounts
    v = np.asarray(scorer.ps.p.cpu().numpy(), np.float64) * scorer.y_scale + scorer.y_shift
    tg = []
    for _ in range(max(rounds, 3)):
        t0 = time.perf_counter()
        group_sums_host(v, grp.ids, G)
        tg.append(time.perf_counter() - t0)
    # the D2H copy of the predictions + sync that the host grouping needs first
    tc = [_clock(lambda: scorer.ps.p.cpu())[0] for _ in range(max(rounds, 3))]
    a, b = ps.pieces[0]  # one piece at these sizes
    terms = {"assemble_const_us": [], "assemble_plain_us": [], "forward_us": [], "group_sums_us": []}
    with torch.no_grad():
        for _ in range(max(rounds, 3)):
            terms["assemble_const_us"].append(_events(lambda: ps.assemble(a, b, consts[0])))
            terms["assemble_plain_us"].append(_events(lambda: ps.assemble(a, b)))
            terms["forward_us"].append(_events(lambda: ps.forward(ps.X[: b - a], a)))
            terms["group_sums_us"].append(_events(lambda: grp.reduce(0)))
    rec = {"device": {"pass_s": _median(td), "passes_per_s": 1.0 / _median(td), "all_pass_s": td, "passes_per_window": passes},
           "host": {"pass_s": _median(th), "passes_per_s": 1.0 / _median(th), "all_pass_s": th,
                    "passes_per_window": host_passes},
           "host_grouping_alone_s": _median(tg), "d2h_predictions_s": _median(tc),
           "terms": {k2: _median(v2) * 1e6 for k2, v2 in terms.items()},
           "groups": G, "device_vs_host_rel_diff_of_group_sums": rel, "finite": bool(np.isfinite(sums).all())}
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
    groups, ids = np.unique(np.asarray(table["well"]).astype(str), return_inverse=True)
    ids = ids.reshape(-1).astype(np.int64)
    t_setup, grp = _clock(lambda: GroupSums(LearnedScorer(pred, table, "response"), ids, len(groups)))
    scorer = grp.scorer
    rec = _measure(pred, table, grp, ids, len(groups), passes, host_passes, rounds)
    rec.update(rows=n, features=pipe.n_features, engine_batch=pred.eng_batch, setup_s=t_setup, pieces=len(scorer.ps.pieces))
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
    groups, ids = np.unique(np.asarray(table["well"]).astype(str), return_inverse=True)
    ids = ids.reshape(-1).astype(np.int64)
    t_setup, grp = _clock(lambda: GroupSums(LearnedScorer(pred, table, "response"), ids, len(groups)))
    scorer = grp.scorer
    rec = _measure(pred, table, grp, ids, len(groups), passes, host_passes, rounds)
    pred.eng.check_device_errors()
    rec.update(rows=n, windows=int(scorer.M), features=pipe.n_features, engine_batch=B, setup_s=t_setup)
    return rec


def bench_reductions(M, rounds):
    """group_sums against err_sums on the same M predictions, interleaved windows of 10 launches."""
    from wellflow.ops.native import GroupPlan, err_sums, err_sums_scratch, group_sums

    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    pred = torch.from_numpy(rng.normal(size=M).astype(np.float32)).to(dev)
    y = torch.from_numpy(rng.normal(size=M).astype(np.float32)).to(dev)
    scratch = err_sums_scratch(dev)
    out2 = torch.zeros((1, 2), dtype=torch.float64, device=dev)
    plans = {"g1_grouped": GroupPlan(np.zeros(M, np.int64), 1, dev),
             "g1024_grouped": GroupPlan(np.sort(rng.integers(0, 1024, size=M)), 1024, dev),
             "g1024_scattered": GroupPlan(rng.integers(0, 1024, size=M), 1024, dev)}
    outs = {k: torch.zeros((1, p.G, 3), dtype=torch.float64, device=dev) for k, p in plans.items()}
    fns = {"err_sums": lambda: err_sums(pred, y, 1.5, 0.25, out2, 0, scratch)}
    for k, p in plans.items():
        fns["group_sums_" + k] = (lambda p=p, k=k: group_sums(pred, p, 1.5, 0.25, outs[k], 0))
    for f in fns.values():
        f()
    t = {k: [] for k in fns}
    for _ in range(max(rounds, 5)):
        for k, f in fns.items():  # interleaved: err / g1 / g1024 / scattered / err / ...
            t[k].append(_events(f))
    rec = {k + "_us": _median(v) * 1e6 for k, v in t.items()}
    rec["all_us"] = {k: [x * 1e6 for x in v] for k, v in t.items()}
    rec["M"] = M
    rec["pieces_g1"] = int(plans["g1_grouped"].pieces.shape[1])
    rec["group_sums_g1_over_err_sums"] = rec["group_sums_g1_grouped_us"] / rec["err_sums_us"]
    rec["group_sums_g1024_over_err_sums"] = rec["group_sums_g1024_grouped_us"] / rec["err_sums_us"]
    return rec


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=2_097_152)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--passes", type=int, default=18, help="device passes per timing window")
    ap.add_argument("--host-passes", type=int, default=2, help="host passes per timing window")
    ap.add_argument("--json", default="")
    ap.add_argument("--skip-lstm", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("response_throughput: needs a GPU (no rate is reported without one)", file=sys.stderr)
        return 2
    rec = {"device": torch.cuda.get_device_name(0)}
    with tempfile.TemporaryDirectory() as tmp:
        rec["reductions"] = bench_reductions(args.rows, args.rounds)
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
