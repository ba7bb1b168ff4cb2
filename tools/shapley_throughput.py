#!/usr/bin/env python
"""Exact-Shapley throughput: the fused coalition kernel (csrc/mlp_f32_shap.hip, ``NativeMLP.shapley_f32``)
against the only alternative without it, on the same commit: per coalition, compose the table on
the device (``torch.where(span in S, x, x')``, standing in for an assembly launch) and run
``NativeMLP.forward_f32`` over it, 2^K times.

One process, one engine batch of 64 rows per CU, K = 9 picked columns, random weights and rows.
Interleaved windows (kernel / alternative / kernel ...), each timed with device events; a kernel
window is ``--launches`` launches over all 2^K coalitions, an alternative window is ``--coalitions``
coalitions (compose + forward; the forward alone is timed too: the alternative's floor). Reported per
width: ns per row-coalition of each, their ratio next to the arithmetic's
``65,792 / (256 Fp + 65,792)``, and the kernel's fp32 MFMA rate in its coalition loop.

The share of stage 1 (the K + 1 layer-1 passes, the scratch slab and the sub-group loads) is not
measured inside the kernel: it is estimated from launches at K = 8 and K = 9 with the model
``t(K) = s (K + 1) + c 2^K``, which lumps everything that does not scale with 2^K into ``s``.

    python tools/shapley_throughput.py [--widths 16,72,128,512] [--rounds R] [--json PATH]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from wellflow.models.mlp import MlpLayout, NativeMLP  # noqa: E402
from wellflow.ops.native import lib  # noqa: E402

from throughput_common import _events, _median  # noqa: E402

HID = (256, 256)


def _spans(F: int, K: int):
    """K spans spread over the row, each F / (2 K) features wide (at least 1), gaps between them."""
    w = max(1, F // (2 * K))
    return [c * (F // K) for c in range(K)], [w] * K


def bench_width(F: int, K: int, rounds: int, launches: int, coalitions: int) -> dict:
    dev = torch.device("cuda", 0)
    B = lib().MLP_F32_ROWS * torch.cuda.get_device_properties(dev).multi_processor_count
    g = torch.Generator().manual_seed(F)
    eng = NativeMLP(F, HID, B, device=dev)
    eng.params.copy_((0.1 * torch.randn(MlpLayout(F, HID).numel, generator=g)).to(dev))
    eng.sync_weights()
    X = torch.randn(B, F, generator=g).to(dev)
    xb = X.mean(0).contiguous()
    phi = {k: torch.empty((k, B), dtype=torch.float64, device=dev) for k in (K - 1, K)}
    spans = {k: _spans(F, k) for k in (K - 1, K)}
    member = torch.zeros(K, F, dtype=torch.bool, device=dev)
    for c, (o, n) in enumerate(zip(*spans[K])):
        member[c, o : o + n] = True
    Xi = torch.empty_like(X)

    def kernel(k=K):
        eng.shapley_f32(X, xb, *spans[k], phi[k])

    def alternative(i):
        back = member[[c for c in range(K) if not (i >> c) & 1]].any(0) if i != (1 << K) - 1 else member[0] & False
        torch.where(back[None, :], xb[None, :], X, out=Xi)
        eng.forward_f32(Xi)

    picks = [(37 * j + 5) % (1 << K) for j in range(coalitions)]  # coalitions of mixed sizes

    def alt_window():
        for i in picks:
            alternative(i)

    with torch.no_grad():
        kernel(), kernel(K - 1), alt_window()  # warm-up: both scratch sizes, every path
        tk, tk1, ta, tf = [], [], [], []
        for _ in range(rounds):
            tk.append(_events(kernel, launches))
            ta.append(_events(alt_window, 1) / coalitions)
            tk1.append(_events(lambda: kernel(K - 1), launches))
            tf.append(_events(lambda: eng.forward_f32(X), coalitions))
    eng.check_device_errors()
    t9, t8, alt, fwd = _median(tk), _median(tk1), _median(ta), _median(tf)
    Fp, n = (F + 7) // 8 * 8, 1 << K
    c = (K * t9 - (K + 1) * t8) / (K * n - (K + 1) * (n >> 1))
    s = (t9 - n * c) / (K + 1)
    return {"features": F, "K": K, "rows": B, "kernel_ms": t9 * 1e3, "all_kernel_ms": [t * 1e3 for t in tk],
            "kernel_ns_per_row_coalition": t9 / (B * n) * 1e9,
            "alternative_ns_per_row_coalition": alt / B * 1e9, "forward_only_ns_per_row_coalition": fwd / B * 1e9,
            "ratio_kernel_to_alternative": t9 / n / alt, "ratio_kernel_to_forward_only": t9 / n / fwd,
            "arithmetic_ratio": 65792 / (256 * Fp + 65792),
            "coalition_loop_tflops": 2 * 65792 * B * n / max(t9 - (K + 1) * s, 1e-12) / 1e12,
            "stage1_share_estimate": (K + 1) * s / t9, "kernel_ms_at_K_minus_1": t8 * 1e3,
            "finite": bool(torch.isfinite(phi[K]).all())}


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--widths", default="16,72,128,512")
    ap.add_argument("--columns", type=int, default=9)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=2, help="kernel launches per timing window")
    ap.add_argument("--coalitions", type=int, default=16, help="coalitions per window of the alternative")
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("shapley_throughput: needs a GPU (no rate is reported without one)", file=sys.stderr)
        return 2
    rec = {"device": torch.cuda.get_device_name(0),
           "widths": [bench_width(int(F), args.columns, args.rounds, args.launches, args.coalitions)
                      for F in args.widths.split(",")]}
    line = json.dumps(rec)
    print(line)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
