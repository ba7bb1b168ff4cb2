"""Time of the fp32 path-gradient kernel (NativeMLP.path_gradients_f32, csrc/mlp_f32_path.hip) against
``steps`` launches of NativeMLP.input_gradients_f32 and ``steps`` torch.autograd passes on the same device
rows, and of path_attr (csrc/score.hip) against a device-to-device copy of the same byte traffic.

    python tools/path_throughput.py [--rows 2097152] [--batch 262144] [--widths 16,72,128,512] [--steps 8,32,64]
                                    [--rounds 3]

Per width and step count: seeded normal rows [batch][F] on the device, weights 0.1 * randn, the mean row
as baseline; a pass is rows / batch launches over that buffer (so at narrow widths the rows stay in the
last-level cache: a comparison of launches, not of HBM rates). Device events around a pass, ``--rounds``
windows per route, interleaved path / gradient launches / autograd / path / ...; every route warmed
first. One JSON line per (width, steps): median (min, max) ms per pass, the ratio to the gradient
launches and the expectation 2 / (2 + 2 Fp / 256). Needs a GPU; there is no fallback.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from wellflow.models.mlp import MlpLayout, MLPRegressor, NativeMLP  # noqa: E402
from wellflow.ops.native import lib  # noqa: E402


ATTR_REPEATS = 50  # the path_attr / copy windows: 400 launches, some hundred ms


def timed(fn, passes: int) -> float:
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(passes):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def windows(routes: dict, passes: int, rounds: int) -> dict:
    for fn in routes.values():
        timed(fn, 1)
    ms = {k: [] for k in routes}
    for _ in range(rounds):
        for k, fn in routes.items():
            ms[k].append(timed(fn, passes))
    return {k + "_ms": [round(statistics.median(v), 3), round(min(v), 3), round(max(v), 3)] for k, v in ms.items()}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2097152)
    ap.add_argument("--batch", type=int, default=262144)
    ap.add_argument("--widths", default="16,72,128,512")
    ap.add_argument("--steps", default="8,32,64")
    ap.add_argument("--rounds", type=int, default=3)
    ns = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("path_throughput: needs a GPU")
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
        xb, out = X.mean(0).contiguous(), torch.empty_like(X)
        Fp = (F + 7) // 8 * 8

        def autograd():
            x = X.detach().requires_grad_(True)
            torch.autograd.grad(ref(x).sum(), x)

        # path_attr over 8 equal spans against a copy that moves the same bytes: path_attr reads X and avg and
        # writes phi (K x 8 B per row); a copy reads and writes its buffer, so the buffer is HALF that total.
        # The pair is short (a few ms per pass), so a window repeats the pass ATTR_REPEATS times.
        K = min(8, F)
        off = torch.arange(K, dtype=torch.int32, device=dev) * (F // K)
        size = torch.full((K,), F // K, dtype=torch.int32, device=dev)
        phi = torch.empty((K, ns.batch), dtype=torch.float64, device=dev)
        src = torch.empty((2 * X.numel() + 2 * phi.numel()) // 2, device=dev)
        dst = torch.empty_like(src)
        attr = windows({"path_attr": lambda: lib().path_attr(X, out, xb, F, off, size, phi, 0),
                        "d2d_copy": lambda: dst.copy_(src)}, passes * ATTR_REPEATS, ns.rounds)
        attr = {k: [round(t / ATTR_REPEATS, 4) for t in v] for k, v in attr.items()}
        print(json.dumps({"F": F, "rows": passes * ns.batch, "spans": K, **attr,
                          "attr_over_copy": round(attr["path_attr_ms"][0] / attr["d2d_copy_ms"][0], 3)}), flush=True)
        for m in (int(s) for s in ns.steps.split(",")):
            def launches():
                for _ in range(m):
                    eng.input_gradients_f32(X, out)

            def autograds():
                for _ in range(m):
                    autograd()

            res = windows({"path_kernel": lambda: eng.path_gradients_f32(X, xb, m, out), "grad_launches": launches,
                           "torch_autograd": autograds}, passes, ns.rounds)
            eng.check_device_errors()
            res["path_over_launches"] = round(res["path_kernel_ms"][0] / res["grad_launches_ms"][0], 3)
            res["expected"] = round(2 / (2 + 2 * Fp / 256), 3)
            res["autograd_over_path"] = round(res["torch_autograd_ms"][0] / res["path_kernel_ms"][0], 3)
            print(json.dumps({"F": F, "steps": m, "rows": passes * ns.batch, "batch": ns.batch, "rounds": ns.rounds,
                              **res}), flush=True)
        del eng, ref, X, out
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
