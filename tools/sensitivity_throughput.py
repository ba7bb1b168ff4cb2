"""Time of the fp32 input-gradient kernel (NativeMLP.input_gradients_f32, csrc/mlp_f32_grad.hip)
against NativeMLP.forward_f32 and torch.autograd on the same device rows.

    python tools/sensitivity_throughput.py [--rows 2097152] [--batch 262144] [--widths 16,72,128,512] [--rounds 5]

Per width: seeded normal rows [batch][F] on the device, weights 0.1 * randn; a pass is rows / batch
launches over that buffer (so at narrow widths the rows stay in the last-level cache: a comparison
of launches, not of HBM rates). Device events around a pass, ``--rounds`` windows per route,
interleaved kernel / forward / autograd / kernel / ...; every route warmed first. One JSON line per
width: median (min, max) ms per pass. Needs a GPU; there is no fallback.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from wellflow.models.mlp import MlpLayout, MLPRegressor, NativeMLP  # noqa: E402


def timed(fn, passes: int) -> float:
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(passes):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2097152)
    ap.add_argument("--batch", type=int, default=262144)
    ap.add_argument("--widths", default="16,72,128,512")
    ap.add_argument("--rounds", type=int, default=5)
    ns = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sensitivity_throughput: needs a GPU")
    dev, passes = torch.device("cuda", 0), max(1, ns.rows // ns.batch)
    for F in (int(w) for w in ns.widths.split(",")):
        g = torch.Generator().manual_seed(F)
        flat = 0.1 * torch.randn(MlpLayout(F, (256, 256)).numel, generator=g)
        eng = NativeMLP(F, (256, 256), ns.batch, device=dev)
        eng.params.copy_(flat.to(dev))
        eng.sync_weights()
        ref = MLPRegressor(F, (256, 256))
        ref.load_flat(flat)
        ref = ref.to(dev)
        X = torch.randn(ns.batch, F, generator=g).to(dev)
        dX = torch.empty_like(X)

        def autograd():
            x = X.detach().requires_grad_(True)
            torch.autograd.grad(ref(x).sum(), x)

        routes = {"grad_kernel": lambda: eng.input_gradients_f32(X, dX), "forward_f32": lambda: eng.forward_f32(X),
                  "torch_autograd": autograd}
        for fn in routes.values():
            timed(fn, 2)
        ms = {k: [] for k in routes}
        for _ in range(ns.rounds):
            for k, fn in routes.items():
                ms[k].append(timed(fn, passes))
        eng.check_device_errors()
        out = {"F": F, "rows": passes * ns.batch, "batch": ns.batch, "rounds": ns.rounds}
        for k, v in ms.items():
            out[k + "_ms"] = [round(statistics.median(v), 3), round(min(v), 3), round(max(v), 3)]
        out["grad_over_forward"] = round(out["grad_kernel_ms"][0] / out["forward_f32_ms"][0], 3)
        out["autograd_over_grad"] = round(out["torch_autograd_ms"][0] / out["grad_kernel_ms"][0], 3)
        print(json.dumps(out), flush=True)
        del eng, ref, X, dX
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
