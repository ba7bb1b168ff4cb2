"""What the ``*_throughput.py`` tools share: the wall clock around a synchronised call, the median,
device-event timing of a launch, and a bf16 predictor on the GPU from a freshly saved model."""
from __future__ import annotations

import os
import time

import numpy as np
import torch

from wellflow.models import registry
from wellflow.predict import Predictor
from wellflow.utils.checkpoint import save_mdl


def _clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def _median(v):
    return float(np.median(np.asarray(v, np.float64)))


def _events(fn, launches=10):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / launches * 1e-3


def _predictor(tmp, name, ref, pipe, schema, job=None, batch=0):
    p = os.path.join(tmp, "models", f"{name}.mdl")
    extra = {"features": pipe.state()}
    if job:
        extra["job"] = job
    save_mdl(p, name, registry.keras_layers(name, ref), extra)
    return Predictor.load(p, schema, device="cuda", precision="bf16", batch=batch)
