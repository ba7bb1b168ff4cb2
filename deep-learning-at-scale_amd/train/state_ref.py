"""What a training job carries on the device from one step to the next, declared per class.

A ``.ckpt`` (Trainer.state_dict) holds the flat fp32 parameters, the optimizer's moments and two
integers. On the GPU a running job reads much more: the bf16 operand images of the weights, the
device step counter, the CNN's dropout counter. A resume is right only when all of it comes back
bit for bit. This module sorts EVERY tensor attribute of the native engines, their
SmallLaunchState and the flat optimizers into exactly one of four classes, so the resume tests
(tests/test_resume_gpu.py) compare the right set and a buffer added later cannot go unclassified
(:func:`unclassified`; tests/test_resume_cpu.py).

* CARRIED   written by a training step and read by a later one; identical after a restore.
* REBUILT   a pure function of carried state (the bf16 operand images): a running job gets them
            from the fused updates, a resumed one from ``sync_weights``. Compared like CARRIED.
* SCRATCH   fully written before it is read within one step or one launch. Never compared.
* FIXED     constructor constants and synchronisation words. Never compared, never written by a
            test: sync words, tickets, launch epochs, STAT blocks, and the clip state block
            (``clip_state[0]``, the factor, is recomputed before every read; ``[1:4]`` are
            per-epoch statistics that are deliberately NOT carried over a resume; ``[4]`` is a
            ticket).

Two buffers are mixed and are listed under the class of what a later step reads from them:
``step_dev`` is CARRIED for word 0 (the step count; only that word is compared) while word 1 is
the update kernel's completion ticket (0 between steps, asserted by the tests on its own);
``XH`` / ``Cst`` of the LSTM are SCRATCH whose ``h_init`` / ``c_init`` block stays the
constructor's zero, and ``ypad`` of the CNN's GEMM path is SCRATCH whose padding columns do.
"""
from __future__ import annotations

import torch

CARRIED, REBUILT, SCRATCH, FIXED = "carried", "rebuilt", "scratch", "fixed"

STATE_CLASSES = {
    "NativeMLP": {
        "params": CARRIED, "grads": CARRIED,  # the bucket: all zero between steps (zero_grads)
        "shadow": REBUILT, "w2t": REBUILT,
        "X": SCRATCH, "_Xop": SCRATCH, "Hs": SCRATCH, "dZ": SCRATCH, "pred": SCRATCH, "dy": SCRATCH,
        "loss_sum": SCRATCH, "M2": SCRATCH, "red": SCRATCH,
    },
    "NativeLSTM": {
        "params": CARRIED, "grads": CARRIED,
        "Wp": REBUILT, "WhhT": REBUILT,
        "XH": SCRATCH, "Cst": SCRATCH, "S": SCRATCH, "DG": SCRATCH, "dcarry": SCRATCH, "pred": SCRATCH,
        "dy": SCRATCH, "loss_sum": SCRATCH, "dw_slab": SCRATCH,
        "sync": FIXED, "sync_bwd": FIXED,
    },
    "NativeCNN": {
        "params": CARRIED, "grads": CARRIED, "rng": CARRIED,
        "WcA": REBUILT, "WdF": REBUILT, "WdB": REBUILT, "shadow": REBUILT,  # shadow: the GEMM path
        "loss_sum": SCRATCH, "dout": SCRATCH, "pred": SCRATCH, "part_wd": SCRATCH, "part_wc": SCRATCH,
        "part_f": SCRATCH, "Xcol": SCRATCH, "Hc": SCRATCH, "dZc": SCRATCH, "ypad": SCRATCH, "dpred": SCRATCH,
    },
    "SmallLaunchState": {"scratch": SCRATCH, "sync": FIXED},
    # params / grads / shadow / shadow_t are the engine's own tensors (compared once, under the
    # engine's names)
    "FlatAdam": {
        "params": CARRIED, "grads": CARRIED, "m": CARRIED, "v": CARRIED, "step_dev": CARRIED,
        "shadow": REBUILT, "shadow_t": REBUILT,
        "clip_scratch": SCRATCH, "clip_state": FIXED,
    },
    "FlatSGD": {
        "params": CARRIED, "grads": CARRIED, "vel": CARRIED, "step_dev": CARRIED,
        "clip_scratch": SCRATCH, "clip_state": FIXED,
    },
}


def _tensors(value) -> list:
    """The tensors an attribute holds: itself, or the tensor members of a list / tuple
    (NativeMLP.Hs, FlatAdam.shadow_t)."""
    if torch.is_tensor(value):
        return [value]
    if isinstance(value, (list, tuple)):
        return [t for t in value if torch.is_tensor(t)]
    return []


def tensor_attributes(obj) -> dict:
    """{attribute name: [tensors]} of every instance attribute of ``obj`` that holds a tensor."""
    return {k: ts for k, ts in ((k, _tensors(v)) for k, v in vars(obj).items()) if ts}


def _parts(eng, opt) -> list:
    small = getattr(eng, "small", None)
    return [o for o in (eng, small, opt) if o is not None]


def unclassified(eng, opt=None) -> list:
    """"Class.attribute" of every tensor attribute of the engine, its SmallLaunchState and the
    optimizer that STATE_CLASSES does not sort into a class ([] when the declaration is complete)."""
    out = []
    for o in _parts(eng, opt):
        known = STATE_CLASSES.get(type(o).__name__, {})
        out += [f"{type(o).__name__}.{k}" for k in tensor_attributes(o) if k not in known]
    return sorted(out)


def images(eng) -> list:
    """Names of the engine's REBUILT buffers that exist: what sync_weights has to write on a resume."""
    known = STATE_CLASSES[type(eng).__name__]
    return sorted(k for k in tensor_attributes(eng) if known.get(k) == REBUILT)


def device_state(eng, opt) -> dict:
    """The CARRIED and REBUILT tensors of an engine and its optimizer, cloned, by attribute name.
    A tensor that engine and optimizer share (params, grads, the MLP's shadow / W2^T) appears
    once, under the engine's name; ``step_dev`` is its word 0, the step count."""
    if eng.device.type == "cuda":
        torch.cuda.synchronize(eng.device)
    out, seen = {}, set()
    for o in _parts(eng, opt):
        known = STATE_CLASSES.get(type(o).__name__, {})
        for name, ts in tensor_attributes(o).items():
            if known.get(name) not in (CARRIED, REBUILT):
                continue
            for i, t in enumerate(ts):
                if t.data_ptr() in seen:
                    continue
                seen.add(t.data_ptr())
                key = name if len(ts) == 1 else f"{name}[{i}]"
                assert key not in out, key
                out[key] = (t[:1] if name == "step_dev" else t).detach().clone()
    return out


_BITS = {1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Equal dtype, shape and bit pattern (bf16 read as int16, fp32 as int32: a NaN equals the
    same NaN, -0.0 does not equal +0.0)."""
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.device != b.device:
        a, b = a.cpu(), b.cpu()
    it = _BITS[a.element_size()]
    return bool(torch.equal(a.contiguous().view(it), b.contiguous().view(it)))


def compare_states(a: dict, b: dict) -> list:
    """Names whose tensors differ by bit pattern between two :func:`device_state` dicts, sorted;
    a name only one side has differs."""
    return sorted(k for k in set(a) | set(b) if k not in a or k not in b or not same_bits(a[k], b[k]))
