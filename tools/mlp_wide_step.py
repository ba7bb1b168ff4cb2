"""Time NativeMLP.forward_backward at 64 < Fp <= 512: the fused wide step (wide_step = True) against
the per-layer route it replaces (wide_step = False, the code path as it was), with and without rows=.

    python tools/mlp_wide_step.py [--rounds 7] [--calls 5] [--loss mse|mae_clip]

One engine per width at B = NativeMLP.full_batch(device). Device events around ``--calls`` calls per
window; windows interleaved wide / per-layer / wide / ...; both routes warmed at every width first.
Prints one line per (Fp, rows) with the medians and the min-max spread in ms."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from wellflow.models.mlp import NativeMLP, init_mlp_flat  # noqa: E402


def window(eng, x, y, rows, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        eng.forward_backward(x, y, 1.0 / eng.B, rows=rows)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--widths", default="72,128,256,512")
    ap.add_argument("--loss", default="mse", choices=["mse", "mae_clip"])
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    B = NativeMLP.full_batch(dev)
    for F in (int(w) for w in args.widths.split(",")):
        eng = NativeMLP(F, (256, 256), B, device=dev, loss=args.loss)
        eng.params.copy_(init_mlp_flat(F).to(dev))
        eng.sync_weights()
        g = torch.Generator(device="cpu").manual_seed(F)
        x = eng.to_input_format(torch.randn(B, F, generator=g)).to(dev)
        y = torch.randn(B, generator=g).to(dev)
        perm = torch.randperm(B, generator=g).to(dev)
        for rows in (None, perm):
            t = {True: [], False: []}
            for wide in (True, False):  # warm both routes
                eng.wide_step = wide
                window(eng, x, y, rows, 2)
            for _ in range(args.rounds):
                for wide in (True, False):
                    eng.wide_step = wide
                    t[wide].append(window(eng, x, y, rows, args.calls))
            eng.wide_step = True
            med = {k: statistics.median(v) for k, v in t.items()}
            print(f"{args.loss} Fp={eng.Fp} rows={'yes' if rows is not None else 'no'} B={B}: wide {med[True]:.3f} ms "
                  f"({min(t[True]):.3f}-{max(t[True]):.3f}), per-layer {med[False]:.3f} ms "
                  f"({min(t[False]):.3f}-{max(t[False]):.3f}), per-layer / wide {med[False] / med[True]:.2f}", flush=True)
        del eng, x, y, perm
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
