#!/usr/bin/env python
"""Set-point throughput: ms per scan pass and per refine pass of the device pass loop
(wellflow/setpoint.py) against what a user could do without it — replace the column on the host,
call ``Predictor.predict_table`` once per pass, then run the numpy rule — on the same commit.

One process, interleaved timing windows (device scan / device refine / host scan / host refine /
...), so every variant sees the same machine state. The shape: MLP 16-256-256-1 on an in-memory
synthetic table of N = 2,097,152 rows (6 wells: 6 + 3 one-hot columns + 7 continuous), the column
``choke`` searched for the row's recorded flow.

A device window is ``--passes`` passes of the pass loop with ONE synchronisation at its end (the
job's shape: the host reads the state once); a host window is ``--host-passes`` passes of host
replace + ``predict_table`` + ``solve_step_host``. The terms of a device pass (constant assembly,
per-row assembly, forward, solve_step) are timed alone with device events, 10 launches per window;
``solve_step`` (scan and refine) against a device-to-device copy of the bytes it moves, and the
``perm_values`` launch of the assembly kernel against the plain launch, interleaved.

    python tools/setpoint_throughput.py [--rows N] [--rounds R] [--json PATH]
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
from wellflow.scoring import RowValues, constant  # noqa: E402
from wellflow.setpoint import FIRST, REFINE, SCAN, BracketSearch, new_state, solve_step_host  # noqa: E402
from wellflow.whatif import LearnedScorer  # noqa: E402

from throughput_common import _clock, _events, _median, _predictor  # noqa: E402

NAMES = "well,field,t,whp,choke,glr,temp,water_cut,dsp,flow"
TYPES = "string,string,int,float,float,float,float,float,float,float"


def bench_mlp(rows, passes, host_passes, rounds, tmp):
    from wellflow.models.mlp import MLPRegressor

    schema = parse_schema(NAMES, TYPES)
    wells = 6  # 6 well + 3 field one-hot columns + 7 continuous = 16 features
    table = load_table("synth", schema, synth_wells=wells, synth_steps=(rows + wells - 1) // wells, seed=1)
    table = take(table, np.arange(rows))
    n = len(table["flow"])
    pipe = FeaturePipeline(schema, "flow", standardize_target=True).fit(take(table, np.arange(0, n, 32)))
    torch.manual_seed(0)
    pred = _predictor(tmp, "mlp", MLPRegressor(pipe.n_features, (256, 256)), pipe, schema)
    want = np.asarray(table["flow"], np.float32)
    t_setup, scorer = _clock(lambda: LearnedScorer(pred, table, "set-point"))
    ps = scorer.ps
    k = ps.names.index("choke")
    search = BracketSearch(scorer, k, want)
    lo, hi = float(np.min(table["choke"])), float(np.max(table["choke"]))
    grid = np.linspace(lo, hi, passes, dtype=np.float64).astype(np.float32)
    consts = search.constants(grid)  # the one upload of the grid

    def device_scan():
        with torch.no_grad():
            for g, c in enumerate(consts):
                search.scan(g, c)
        return search.finish()  # the one read of the state

    def device_refine():
        with torch.no_grad():
            for _ in range(passes):
                search.refine()
        return search.finish()

    hxs, hfs, hst = new_state(n)

    def host_pass(edit_table, mode, x):
        p = np.asarray(pred.predict_table(edit_table), np.float64)
        # predict_table returns raw units: the rule's residual with y_scale = 1, y_shift = 0
        solve_step_host(p, want, 1.0, 0.0, mode, x, hxs, hfs, hst)

    def host_scan():
        for g in range(host_passes):
            host_pass(constant(table, "choke", grid[g]), FIRST if g == 0 else SCAN, grid[g])

    def host_refine():
        for _ in range(host_passes):
            t2 = dict(table)
            t2["choke"] = hxs[3].copy()
            host_pass(t2, REFINE, None)

    with torch.no_grad():
        search.baseline()
    device_scan()  # warm-up of every path
    device_refine()
    host_scan()
    host_refine()
    t = {"device_scan": [], "device_refine": [], "host_scan": [], "host_refine": []}
    for _ in range(rounds):
        t["device_scan"].append(_clock(device_scan)[0] / passes)
        t["device_refine"].append(_clock(device_refine)[0] / passes)
        t["host_scan"].append(_clock(host_scan)[0] / host_passes)
        t["host_refine"].append(_clock(host_refine)[0] / host_passes)
    xs, fs, status, _ = search.finish()
    a, b = ps.pieces[0]  # one piece at these sizes
    row_edit = RowValues(k, search.xs[3], search.ident)
    terms = {"assemble_const_us": [], "assemble_rows_us": [], "assemble_plain_us": [], "forward_us": [],
             "solve_scan_us": [], "solve_refine_us": []}
    with torch.no_grad():
        for _ in range(max(rounds, 3)):
            terms["assemble_const_us"].append(_events(lambda: ps.assemble(a, b, consts[1])))
            terms["assemble_rows_us"].append(_events(lambda: ps.assemble(a, b, row_edit)))
            terms["assemble_plain_us"].append(_events(lambda: ps.assemble(a, b)))
            terms["forward_us"].append(_events(lambda: ps.forward(ps.X[: b - a], a)))
            terms["solve_scan_us"].append(_events(lambda: search.step(ps.p, SCAN, 1)))
            terms["solve_refine_us"].append(_events(lambda: search.step(ps.p, REFINE)))
    rec = {k2: {"pass_ms": _median(v) * 1e3, "all_pass_ms": [x * 1e3 for x in v]} for k2, v in t.items()}
    rec.update(passes_per_window=passes, host_passes_per_window=host_passes,
               terms={k2: _median(v2) * 1e6 for k2, v2 in terms.items()},
               scan_speedup=_median(t["host_scan"]) / _median(t["device_scan"]),
               refine_speedup=_median(t["host_refine"]) / _median(t["device_refine"]),
               rows=n, features=pipe.n_features, engine_batch=pred.eng_batch, setup_s=t_setup, pieces=len(ps.pieces),
               bracketed=int((status == 1).sum()), finite=bool(np.isfinite(xs).all()))
    rec["perm_values_over_plain"] = rec["terms"]["assemble_rows_us"] / rec["terms"]["assemble_plain_us"]
    return rec


def bench_solve_step(M, rounds):
    """solve_step alone against a device-to-device copy of the same byte count, interleaved windows
    of 10 launches. A scan of open rows that do not cross reads p, want, status, best_x, best_r and
    f_lo (32 B) and writes lo, hi, f_lo, f_hi and xq (28 B; 12 B more where a row improves): 60 B per
    row, the figure the copy moves (30 B read + 30 B written per row). A refine of bracketed rows
    reads p, want, status, xq, f_lo, lo and hi (32 B) and writes one end, its residual and xq (16 B):
    48 B per row."""
    from wellflow.ops.native import SOLVE_FIRST, SOLVE_REFINE, SOLVE_SCAN, solve_step

    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    w = rng.normal(size=M).astype(np.float32)
    gap = 1.0 + np.abs(rng.normal(size=M))
    want = torch.from_numpy(w).to(dev)
    ps = [torch.from_numpy((w + gap).astype(np.float32)).to(dev),   # all above: the rows stay open
          torch.from_numpy((w - gap).astype(np.float32)).to(dev)]   # all below: every row brackets
    xs = torch.zeros((4, M), dtype=torch.float32, device=dev)
    fs = torch.zeros((3, M), dtype=torch.float64, device=dev)
    st = torch.zeros(M, dtype=torch.int32, device=dev)
    g = torch.tensor([0.5, 1.5], device=dev)
    src = torch.zeros(30 * M, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    solve_step(ps[0], want, 1.0, 0.0, SOLVE_FIRST, g[0:1], xs, fs, st)
    fns = {"solve_scan_open": lambda: solve_step(ps[0], want, 1.0, 0.0, SOLVE_SCAN, g[1:2], xs, fs, st),
           "copy_60B_per_row": lambda: dst.copy_(src)}
    for f in fns.values():
        f()
    t = {k: [] for k in ("solve_scan_open", "copy_60B_per_row", "solve_refine")}
    for _ in range(max(rounds, 5)):
        for k, f in fns.items():
            t[k].append(_events(f))
    solve_step(ps[1], want, 1.0, 0.0, SOLVE_SCAN, g[1:2], xs, fs, st)  # every row brackets
    assert int(st.sum()) == M
    fns = {"solve_refine": lambda: solve_step(ps[0], want, 1.0, 0.0, SOLVE_REFINE, None, xs, fs, st),
           "copy_60B_per_row": lambda: dst.copy_(src)}
    for _ in range(max(rounds, 5)):
        for k, f in fns.items():
            t[k].append(_events(f))
    rec = {k + "_us": _median(v) * 1e6 for k, v in t.items()}
    rec["M"] = M
    rec["solve_scan_over_copy"] = rec["solve_scan_open_us"] / rec["copy_60B_per_row_us"]
    rec["solve_refine_over_copy"] = rec["solve_refine_us"] / rec["copy_60B_per_row_us"]
    rec["copy_GBps"] = 60.0 * M / rec["copy_60B_per_row_us"] * 1e-3
    rec["solve_scan_GBps"] = 60.0 * M / rec["solve_scan_open_us"] * 1e-3
    rec["solve_refine_GBps"] = 48.0 * M / rec["solve_refine_us"] * 1e-3
    return rec


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=2_097_152)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--passes", type=int, default=12, help="device passes per timing window")
    ap.add_argument("--host-passes", type=int, default=2, help="host passes per timing window")
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("setpoint_throughput: needs a GPU (no rate is reported without one)", file=sys.stderr)
        return 2
    rec = {"device": torch.cuda.get_device_name(0)}
    with tempfile.TemporaryDirectory() as tmp:
        rec["solve_step"] = bench_solve_step(args.rows, args.rounds)
        rec["mlp"] = bench_mlp(args.rows, args.passes, args.host_passes, args.rounds, tmp)
    line = json.dumps(rec)
    print(line)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
