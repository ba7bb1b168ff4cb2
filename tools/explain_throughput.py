#!/usr/bin/env python
"""Shapley-attribution throughput: ms per pass of the device pass loop (wellflow/explain.py) against
what a user could do before it — permute the set's columns on the host, call
``Predictor.predict_table`` once per pass and accumulate per row in numpy — on the same commit.

One process, interleaved timing windows (device / host / device / host ...), so both variants see
the same machine state. Two shapes, those of tools/importance_throughput.py:

* MLP 16-256-256-1 on an in-memory synthetic table of N = 2,097,152 rows (6 wells: 6 + 3 one-hot
  columns + 7 continuous);
* LSTM (H = 512, T = 64) at its full-grid batch, 8 full chunks of windows.

A device window is ``--repeats`` repeats of the job's loop (K passes each: the draw of the row
map, the start pass, K - 1 steps, the last step on the kept p_full) with ONE synchronisation at
its end; the read of the fp64 tables, which the job does once, is timed on its own. A host window
is ``--host-passes`` passes of host permute + ``predict_table`` + numpy accumulation. The terms of
a device pass are also timed alone with device events, 10 launches per window: randperm, the set
assembly at set sizes 1, K / 2 and K (random and cyclic-shift row maps) next to the plain launch,
the forward(s), attr_step next to a device-to-device copy that moves the same number of bytes.

    python tools/explain_throughput.py [--rows N] [--rounds R] [--json PATH]
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
from wellflow.explain import Attribution  # noqa: E402
from wellflow.ops.native import attr_step  # noqa: E402
from wellflow.scoring import PermutedSet  # noqa: E402
from wellflow.whatif import LearnedScorer  # noqa: E402

from throughput_common import _clock, _events, _median, _predictor  # noqa: E402

NAMES = "well,field,t,whp,choke,glr,temp,water_cut,dsp,flow"
TYPES = "string,string,int,float,float,float,float,float,float,float"


def _measure(pred, table, att, repeats, host_passes, rounds, cyclic):
    """Interleaved device / host windows over all input columns."""
    scorer = att.scorer
    ps = scorer.ps  # the pass (wellflow/scoring.py): its own assembly and forward steps are timed below
    n = len(table["flow"])
    dev = pred.device
    names = ps.names
    K = len(names)
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    rng = np.random.default_rng(0)
    order = rng.permutation(K)
    sets = att.column_sets([[int(k) for k in order[j:]] for j in range(K)], K)  # the passes of one repeat
    ar = torch.arange(n, device=dev, dtype=torch.int32)
    att.begin(K)

    def draw():
        if cyclic:  # the LSTM's default row map
            return (ar + int(rng.integers(1, n))) % n
        return torch.randperm(n, generator=gen, device=dev, dtype=torch.int32)

    def device_window():
        with torch.no_grad():
            for _ in range(repeats):
                perm = draw()
                att.step(sets[0], perm, K, True)
                for j in range(K - 1):
                    att.step(sets[j + 1], perm, int(order[j]), False)
                att.last(int(order[K - 1]))

    ys, sh = scorer.y_scale, scorer.y_shift
    rows = np.arange(n) if ps.rows is None else ps.rows

    def host_window():
        acc, prev = np.zeros(len(rows)), None
        for i in range(host_passes):
            perm = rng.permutation(n)
            t2 = dict(table)
            for k in order[i % K:]:
                t2[names[k]] = np.asarray(table[names[k]])[perm]
            p = np.asarray(pred.predict_table(t2), np.float64)[rows]
            if prev is not None:
                d = p - prev
                acc += d
                acc += d * d  # the second table's update: the same traffic
            prev = p
        return acc

    with torch.no_grad():
        att.full()
    device_window()  # warm-up of both paths
    host_window()
    td, th = [], []
    for _ in range(rounds):
        td.append(_clock(device_window)[0] / (repeats * K))
        th.append(_clock(host_window)[0] / host_passes)
    t_read, (acc, sq, _) = _clock(att.finish)  # the one read of the tables
    # the terms of one device pass, each alone
    a, b = ps.pieces[0]  # one piece at these sizes
    M = scorer.M
    perm_r = torch.randperm(n, generator=gen, device=dev, dtype=torch.int32)
    perm_c = (ar + n // 3) % n
    sizes = {"1": sets[K - 1], "half": sets[K - K // 2], "all": sets[0]}
    assert [len(host) for host, _ in sizes.values()] == [1, K // 2, K]
    copy_src = torch.empty(22 * M, dtype=torch.uint8, device=dev)  # attr_step moves 44 B per cell: 24 read, 20 written
    copy_dst = torch.empty_like(copy_src)
    terms = {"randperm": [], "assemble_plain": [], "forward": [], "attr_step": [], "copy_same_bytes": []}
    for s in sizes:
        terms[f"assemble_set_{s}_random"], terms[f"assemble_set_{s}_cyclic"] = [], []
    with torch.no_grad():
        for _ in range(max(rounds, 3)):
            terms["randperm"].append(_events(lambda: torch.randperm(n, generator=gen, device=dev, dtype=torch.int32)))
            terms["assemble_plain"].append(_events(lambda: ps.assemble(a, b)))
            for s, cs in sizes.items():
                er, ec = PermutedSet(*cs, perm_r), PermutedSet(*cs, perm_c)
                terms[f"assemble_set_{s}_random"].append(_events(lambda: ps.assemble(a, b, er)))
                terms[f"assemble_set_{s}_cyclic"].append(_events(lambda: ps.assemble(a, b, ec)))
            terms["forward"].append(_events(lambda: ps.forward(ps.X[: b - a], a)))
            terms["attr_step"].append(_events(lambda: attr_step(ps.p, att.p_prev, ys, sh, att.acc, att.sq, 0)))
            terms["copy_same_bytes"].append(_events(lambda: copy_dst.copy_(copy_src)))
    us = {k: _median(v) * 1e6 for k, v in terms.items()}
    res = ps.res
    src_bytes = (res.C + res.Q) * 4 * (b - a)
    out_bytes = (b - a) * ps.X.shape[1] * ps.X.element_size()
    gbs = {k: (src_bytes + out_bytes + (0 if k == "assemble_plain" else 4 * (b - a))) / (v * 1e-6) / 1e9
           for k, v in us.items() if k.startswith("assemble")}
    gbs["attr_step"] = 44 * M / (us["attr_step"] * 1e-6) / 1e9
    gbs["copy_same_bytes"] = 44 * M / (us["copy_same_bytes"] * 1e-6) / 1e9
    rec = {"device": {"pass_ms": _median(td) * 1e3, "all_pass_ms": [t * 1e3 for t in td], "passes_per_window": repeats * K},
           "host": {"pass_ms": _median(th) * 1e3, "all_pass_ms": [t * 1e3 for t in th], "passes_per_window": host_passes},
           "read_tables_ms": t_read * 1e3, "terms_us": us, "gb_per_s": gbs, "columns": K, "predictions": int(M),
           "row_map": "cyclic shift" if cyclic else "randperm", "finite": bool(np.isfinite(acc).all() and np.isfinite(sq).all())}
    rec["speedup"] = rec["host"]["pass_ms"] / rec["device"]["pass_ms"]
    return rec


def bench_mlp(rows, repeats, host_passes, rounds, tmp):
    from wellflow.models.mlp import MLPRegressor

    schema = parse_schema(NAMES, TYPES)
    wells = 6  # 6 well + 3 field one-hot columns + 7 continuous = 16 features
    table = load_table("synth", schema, synth_wells=wells, synth_steps=(rows + wells - 1) // wells, seed=1)
    table = take(table, np.arange(rows))  # the last well is a few rows short; every well is still there
    n = len(table["flow"])
    pipe = FeaturePipeline(schema, "flow", standardize_target=True).fit(take(table, np.arange(0, n, 32)))
    torch.manual_seed(0)
    pred = _predictor(tmp, "mlp", MLPRegressor(pipe.n_features, (256, 256)), pipe, schema)
    t_setup, att = _clock(lambda: Attribution(LearnedScorer(pred, table, "attribution")))
    scorer = att.scorer
    rec = _measure(pred, table, att, repeats, host_passes, rounds, cyclic=False)
    rec.update(rows=n, features=pipe.n_features, engine_batch=pred.eng_batch, setup_s=t_setup, pieces=len(scorer.ps.pieces))
    return rec


def bench_lstm(repeats, host_passes, rounds, tmp):
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
    t_setup, att = _clock(lambda: Attribution(LearnedScorer(pred, table, "attribution")))
    scorer = att.scorer
    rec = _measure(pred, table, att, repeats, host_passes, rounds, cyclic=True)
    pred.eng.check_device_errors()
    rec.update(rows=n, features=pipe.n_features, engine_batch=B, setup_s=t_setup)
    return rec


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=2_097_152)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=2, help="repeats (K passes each) per device timing window")
    ap.add_argument("--host-passes", type=int, default=2, help="host passes per timing window")
    ap.add_argument("--json", default="")
    ap.add_argument("--skip-lstm", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("explain_throughput: needs a GPU (no rate is reported without one)", file=sys.stderr)
        return 2
    rec = {"device": torch.cuda.get_device_name(0)}
    with tempfile.TemporaryDirectory() as tmp:
        rec["mlp"] = bench_mlp(args.rows, args.repeats, args.host_passes, args.rounds, tmp)
        if not args.skip_lstm:
            rec["lstm"] = bench_lstm(args.repeats, args.host_passes, args.rounds, tmp)
    line = json.dumps(rec)
    print(line)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
