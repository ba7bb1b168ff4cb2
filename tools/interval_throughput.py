#!/usr/bin/env python
"""Calibration-reduction throughput of the prediction-interval job (wellflow/interval.py): the device
reduction that follows the scoring pass -- ``abs_scores``, then ``group_quantiles`` over the ``--by``
plan and over the one-group overall plan (csrc/quantile.hip), then the read of the two small results
-- against the host route the job would otherwise take on the same commit: a D2H copy of the
predictions, the numpy score and an ``np.sort`` per group.

One process, interleaved windows (device / host / copy / device / ...), so every variant sees the
same machine state. The predictions are those of one scoring pass of an MLP 16-256-256-1 over an
in-memory synthetic table of N = 2,097,152 rows; A = 2 levels (0.1, 0.05); G = 1, 6 (the wells:
grouped rows) and 1,024 (scattered ids: the 4-B gather). The device reduction is timed with device
events, 10 launches per window, and once more by the wall clock with the D2H read of the results
(the job's shape). A device-to-device copy of the M fp32 predictions (the bytes the host route's D2H
moves) is timed the same way, as the floor of anything that touches the vector once; the
reduction reads the scores eight times (four rounds, two plans). The plan's one-off host build
(a stable argsort of the ids) is reported apart: a job builds it once.

    python tools/interval_throughput.py [--rows N] [--rounds R] [--json PATH]
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
from wellflow.interval import group_quantiles_host, score_host, select_ranks  # noqa: E402
from wellflow.whatif import LearnedScorer  # noqa: E402

from throughput_common import _clock, _events, _median, _predictor  # noqa: E402

NAMES = "well,field,t,whp,choke,glr,temp,water_cut,dsp,flow"
TYPES = "string,string,int,float,float,float,float,float,float,float"
ALPHAS = ["0.1", "0.05"]


def bench_groups(scorer, y32, ids, G, rounds):
    from wellflow.ops.native import QuantilePlan, abs_scores, group_quantiles

    dev, M, A = scorer.pred.device, int(scorer.M), len(ALPHAS)
    p = scorer.ps.p
    y_dev = torch.from_numpy(y32).to(dev)
    s = torch.empty(M, dtype=torch.float32, device=dev)
    counts = np.bincount(ids, minlength=G)
    r_by, r_all = select_ranks(counts, ALPHAS), select_ranks([M], ALPHAS)
    t_plan, plans = _clock(lambda: (QuantilePlan(ids, G, A, dev), QuantilePlan(np.zeros(M, np.int64), 1, A, dev)))
    ranks = (torch.from_numpy(r_by).to(dev), torch.from_numpy(r_all).to(dev))
    outs = (torch.empty((G, A), device=dev), torch.empty((1, A), device=dev))
    copy = torch.empty_like(p)

    def device():
        abs_scores(p, y_dev, scorer.y_scale, scorer.y_shift, False, s)
        group_quantiles(s, plans[0], ranks[0], outs[0])
        group_quantiles(s, plans[1], ranks[1], outs[1])

    def device_read():
        device()
        return outs[0].cpu().numpy(), outs[1].cpu().numpy()

    def host():
        sh = score_host(p.cpu().numpy(), y32, scorer.y_scale, scorer.y_shift, False)
        return group_quantiles_host(sh, ids, G, r_by), group_quantiles_host(sh, np.zeros(M, np.int64), 1, r_all)

    dq, hq = device_read(), host()  # warm-up of both routes; they agree bit for bit
    same = all(np.array_equal(a.view(np.int32), b.view(np.int32)) for a, b in zip(dq, hq))
    t = {"device_events": [], "device_with_read_wall": [], "host_route_wall": [], "d2d_copy_events": [],
         "abs_scores_events": [], "d2h_predictions_wall": []}
    for _ in range(max(rounds, 3)):
        t["device_events"].append(_events(device))
        t["device_with_read_wall"].append(_clock(device_read)[0])
        t["host_route_wall"].append(_clock(host)[0])
        t["d2d_copy_events"].append(_events(lambda: copy.copy_(p)))
        t["abs_scores_events"].append(_events(lambda: abs_scores(p, y_dev, scorer.y_scale, scorer.y_shift, False, s)))
        t["d2h_predictions_wall"].append(_clock(lambda: p.cpu())[0])
    rec = {k + "_us": _median(v) * 1e6 for k, v in t.items()}
    rec["all_us"] = {k: [x * 1e6 for x in v] for k, v in t.items()}
    rec.update(groups=G, levels=A, M=M, pieces=int(plans[0].groups.pieces.shape[1]), plan_build_s=t_plan,
               device_equals_host_bitwise=bool(same), hist_left_zero=not bool(plans[0].hist.any() or plans[1].hist.any()),
               host_over_device_with_read=rec["host_route_wall_us"] / rec["device_with_read_wall_us"],
               device_over_d2d_copy=rec["device_events_us"] / rec["d2d_copy_events_us"])
    return rec


def main() -> int:
    from wellflow.models.mlp import MLPRegressor

    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=2_097_152)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("interval_throughput: needs a GPU (no rate is reported without one)", file=sys.stderr)
        return 2
    rec = {"device": torch.cuda.get_device_name(0)}
    torch.set_grad_enabled(False)
    schema = parse_schema(NAMES, TYPES)
    wells = 6  # 6 well + 3 field one-hot columns + 7 continuous = 16 features
    table = load_table("synth", schema, synth_wells=wells, synth_steps=(args.rows + wells - 1) // wells, seed=1)
    table = take(table, np.arange(args.rows))
    n = len(table["flow"])
    pipe = FeaturePipeline(schema, "flow", standardize_target=True).fit(take(table, np.arange(0, n, 32)))
    torch.manual_seed(0)
    with tempfile.TemporaryDirectory() as tmp:
        pred = _predictor(tmp, "mlp", MLPRegressor(pipe.n_features, (256, 256)), pipe, schema)
        scorer = LearnedScorer(pred, table, "interval")
        t0 = time.perf_counter()
        with torch.no_grad():
            scorer.predict()
        torch.cuda.synchronize()
        rec.update(rows=n, features=pipe.n_features, engine_batch=pred.eng_batch, first_scoring_pass_s=time.perf_counter() - t0)
        t_pass = [_clock(lambda: scorer.predict())[0] for _ in range(3)]
        rec["scoring_pass_s"] = _median(t_pass)
        y32 = np.asarray(table["flow"], np.float32)
        well_ids = np.unique(np.asarray(table["well"]).astype(str), return_inverse=True)[1].reshape(-1).astype(np.int64)
        rng = np.random.default_rng(0)
        layouts = {"g1": (np.zeros(n, np.int64), 1), "g6_wells": (well_ids, wells),
                   "g1024_scattered": (rng.integers(0, 1024, size=n), 1024)}
        for name, (ids, G) in layouts.items():
            rec[name] = bench_groups(scorer, y32, ids, G, args.rounds)
        pred.eng.check_device_errors()
    line = json.dumps(rec)
    print(line)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
