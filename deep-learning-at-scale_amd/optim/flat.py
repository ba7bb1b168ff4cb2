"""Optimizers over ONE flat fp32 master buffer.

All parameters of a model are views into a single contiguous fp32 tensor and all
gradients into a second one, so an update is one kernel launch (``adam`` / ``sgd`` in
csrc/elementwise.hip) and the data-parallel reduction is one collective on one bucket.
On CPU tensors the same math runs in PyTorch (this is the fp32 oracle path used by the
CPU tests and the parity report — never a silent stand-in for a GPU op).
"""
from __future__ import annotations

import math

import torch


class _GradClip:
    """Keras-0.x gradient clipping (``Optimizer.get_gradients``) for the flat optimizers.

    With g = grads * grad_scale (after the data-parallel all-reduce, so every rank sees the same
    norm and no collective is needed): ``clipnorm = c > 0`` multiplies every element by c / ||g||
    when the L2 norm over the WHOLE bucket is >= c (a non-finite norm leaves g unscaled);
    ``clipvalue = v > 0`` then clamps each element to [-v, v]. 0 = off: no extra launch, and the
    update kernels get no state block.

    On the GPU the norm is one reduction launch in front of the update (csrc/elementwise.hip
    grad_clip_scale_kernel) that leaves the factor in ``clip_state``; the fused update kernels
    read it from there, so a captured step recomputes it on every hipGraph replay. State and
    scratch are allocated once (capture needs fixed addresses)."""

    def _init_clip(self, clipnorm: float, clipvalue: float) -> None:
        self.clipnorm, self.clipvalue = float(clipnorm), float(clipvalue)
        assert self.clipnorm >= 0.0 and self.clipvalue >= 0.0, "clipnorm / clipvalue must be >= 0 (0 = off)"
        # [0] factor [1] norm of the last step [2] clipped steps [3] largest norm [4] ticket
        self.clip_state = self.clip_scratch = None
        if self.params.is_cuda:
            self.clip_state = torch.zeros(8, device=self.params.device)
            self.clip_state[0] = 1.0
            self.clip_scratch = torch.zeros(256, device=self.params.device)
        self._clip_host = {"grad_norm_last": 0.0, "grad_norm_max": 0.0, "clipped_steps": 0}

    @property
    def clips(self) -> bool:
        return self.clipnorm > 0.0 or self.clipvalue > 0.0

    def clip_args(self, grad_scale: float):
        """GPU: launch the norm kernel when clipnorm is on; the (state block | None, clipvalue)
        pair every update binding takes as its trailing arguments."""
        if self.clipnorm <= 0.0:
            return None, self.clipvalue
        from ..ops.native import lib

        lib().grad_clip_scale(self.grads, grad_scale, self.clipnorm, self.clip_scratch, self.clip_state)
        return self.clip_state, self.clipvalue

    def _clipped(self, g: torch.Tensor) -> torch.Tensor:
        """CPU: the same rule in torch (the fp32 oracle). ``g`` = grads * grad_scale."""
        if self.clipnorm > 0.0:
            n = float(torch.linalg.vector_norm(g))
            st = self._clip_host
            st["grad_norm_last"] = n
            st["grad_norm_max"] = n if math.isnan(n) else max(st["grad_norm_max"], n)
            if math.isfinite(n) and n >= self.clipnorm:
                g = g * (self.clipnorm / n)
                st["clipped_steps"] += 1
        if self.clipvalue > 0.0:
            g = g.clamp(-self.clipvalue, self.clipvalue)
        return g

    def clip_stats(self, reset: bool = False) -> dict:
        """``grad_norm_last`` / ``grad_norm_max`` / ``clipped_steps`` since the last reset (the
        norms are recorded while clipnorm is on). One host sync on the GPU."""
        if self.clip_state is not None:
            v = self.clip_state[:4].tolist()
            out = {"grad_norm_last": v[1], "grad_norm_max": v[3], "clipped_steps": int(v[2])}
            if reset:
                self.clip_state[1:4].zero_()
            return out
        out = dict(self._clip_host)
        if reset:
            self._clip_host = {"grad_norm_last": 0.0, "grad_norm_max": 0.0, "clipped_steps": 0}
        return out


class FlatAdam(_GradClip):
    """Adam / AdamW (decoupled weight decay) with PyTorch's bias-correction semantics."""

    def __init__(self, params: torch.Tensor, grads: torch.Tensor, lr: float = 1e-3,
                 betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0,
                 shadow: torch.Tensor | None = None, zero_grads: bool = False, shadow_t=None,
                 writeback=None, clipnorm: float = 0.0, clipvalue: float = 0.0):
        """GPU fusions: ``shadow`` (bf16, same numel) receives the updated weights in the same
        launch (an engine whose compute copy is a plain cast, e.g. NativeMLP.shadow);
        ``shadow_t`` = (bf16 tensor, offset, rows, cols) receives one [rows][cols] block
        transposed in the same launch (NativeMLP.shadow_t: W2^T of the 128-row step kernel);
        ``zero_grads`` clears the gradient bucket after the update (the next
        forward_backward then runs with zero_grads=False); ``writeback``: an engine whose
        ``fused_adam(opt, grad_scale)`` runs this update AND refreshes its compute copies in one
        launch (NativeLSTM: Wp / WhhT), so no sync_weights launch follows (train/step.py)."""
        assert params.dtype == torch.float32 and params.shape == grads.shape
        self.params, self.grads = params, grads
        self.shadow, self.zero_grads = shadow, zero_grads
        self.shadow_t = shadow_t
        self.writeback = writeback
        self.lr, self.betas, self.eps, self.weight_decay = lr, tuple(betas), eps, weight_decay
        self.m = torch.zeros_like(params)
        self.v = torch.zeros_like(params)
        self.t = 0
        # device-side step counter: the GPU update is graph-capturable (bias corrections
        # are computed in-kernel from it, never baked in as launch constants)
        self.step_dev = torch.zeros(4, device=params.device) if params.is_cuda else None
        self._init_clip(clipnorm, clipvalue)

    def step(self, grad_scale: float = 1.0) -> None:
        self.t += 1
        b1, b2 = self.betas
        if self.params.is_cuda:
            from ..ops.native import lib

            wb = self.writeback
            if wb is not None and wb.params is self.params and wb.fused_adam(self, grad_scale):
                return
            st = self.shadow_t or (None, 0, 0, 0)
            lib().adam_dev(self.params, self.grads, self.m, self.v, self.step_dev, self.lr, b1, b2,
                           self.eps, self.weight_decay, grad_scale, self.shadow, self.zero_grads, *st,
                           *self.clip_args(grad_scale))
            return
        bc1, bc2 = 1.0 - b1**self.t, 1.0 - b2**self.t
        g = self._clipped(self.grads * grad_scale)
        self.m.mul_(b1).add_(g, alpha=1 - b1)
        self.v.mul_(b2).addcmul_(g, g, value=1 - b2)
        upd = (self.m / bc1) / ((self.v / bc2).sqrt() + self.eps)
        if self.weight_decay:
            upd = upd + self.weight_decay * self.params
        self.params.sub_(self.lr * upd)
        if self.shadow is not None:
            self.shadow.copy_(self.params)
        if self.shadow_t is not None:
            t, off, r, c = self.shadow_t
            t.view(c, r).copy_(self.params[off : off + r * c].view(r, c).t())
        if self.zero_grads:
            self.grads.zero_()

    @property
    def steps_taken(self) -> int:
        """Updates applied so far. On the GPU the device counter is the truth: hipGraph
        replays (train/step.py) advance it without calling :meth:`step` on the host."""
        if self.step_dev is not None:
            return int(self.step_dev[0].item())
        return self.t

    def state_dict(self) -> dict:
        self.t = self.steps_taken
        return {"kind": "adam", "t": self.t, "m": self.m.detach().cpu(), "v": self.v.detach().cpu(),
                "lr": self.lr, "betas": list(self.betas), "eps": self.eps,
                "weight_decay": self.weight_decay, "clipnorm": self.clipnorm, "clipvalue": self.clipvalue}

    def load_state_dict(self, sd: dict) -> None:
        self.t = int(sd["t"])
        if self.step_dev is not None:
            self.step_dev.zero_()  # [1] is the kernel's completion ticket
            self.step_dev[0] = float(self.t)
        self.m.copy_(sd["m"])
        self.v.copy_(sd["v"])
        self.lr, self.betas, self.eps = sd["lr"], tuple(sd["betas"]), sd["eps"]
        self.weight_decay = sd["weight_decay"]
        # absent in checkpoints written before the optimizers could clip
        self.clipnorm, self.clipvalue = float(sd.get("clipnorm", 0.0)), float(sd.get("clipvalue", 0.0))


class FlatSGD(_GradClip):
    """Keras-0.x SGD (cnn.py:117: lr=0.001, momentum=0.99, decay=1e-6, nesterov=True).

    lr_t = lr / (1 + decay * iterations); v = mu*v - lr_t*g;
    p += mu*v - lr_t*g (Nesterov) else p += v.
    """

    def __init__(self, params: torch.Tensor, grads: torch.Tensor, lr: float = 0.001,
                 momentum: float = 0.99, decay: float = 1e-6, nesterov: bool = True,
                 zero_grads: bool = False, writeback=None, clipnorm: float = 0.0, clipvalue: float = 0.0):
        """``writeback``: an engine whose ``fused_sgd(opt, grad_scale)`` runs this update AND
        refreshes its compute copies in one launch (NativeCNN: the bf16 operand images), so no
        separate sync_weights launch follows (train/step.py StepRunner)."""
        self.params, self.grads = params, grads
        self.writeback = writeback
        self.lr, self.momentum, self.decay, self.nesterov = lr, momentum, decay, nesterov
        self.zero_grads = zero_grads
        self.vel = torch.zeros_like(params)
        self.iterations = 0
        # device iteration counter ([1] = completion ticket): lr_t is computed in-kernel, so a
        # hipGraph-captured update decays the learning rate on every replay
        self.step_dev = torch.zeros(4, device=params.device) if params.is_cuda else None
        self._init_clip(clipnorm, clipvalue)

    def step(self, grad_scale: float = 1.0) -> None:
        if self.params.is_cuda:
            from ..ops.native import lib

            self.iterations += 1
            wb = self.writeback
            if wb is not None and wb.params is self.params and wb.fused_sgd(self, grad_scale):
                return
            lib().sgd_dev(self.params, self.grads, self.vel, self.step_dev, self.lr, self.decay, self.momentum,
                          self.nesterov, grad_scale, self.zero_grads, *self.clip_args(grad_scale))
            return
        lr_t = self.lr / (1.0 + self.decay * self.iterations)
        self.iterations += 1
        g = self._clipped(self.grads * grad_scale)
        self.vel.mul_(self.momentum).sub_(lr_t * g)
        if self.nesterov:
            self.params.add_(self.momentum * self.vel - lr_t * g)
        else:
            self.params.add_(self.vel)
        if self.zero_grads:
            self.grads.zero_()

    @property
    def steps_taken(self) -> int:
        if self.step_dev is not None:
            return int(self.step_dev[0].item())
        return self.iterations

    def state_dict(self) -> dict:
        self.iterations = self.steps_taken
        return {"kind": "sgd", "iterations": self.iterations, "vel": self.vel.detach().cpu(),
                "lr": self.lr, "momentum": self.momentum, "decay": self.decay,
                "nesterov": self.nesterov, "clipnorm": self.clipnorm, "clipvalue": self.clipvalue}

    def load_state_dict(self, sd: dict) -> None:
        self.iterations = int(sd["iterations"])
        if self.step_dev is not None:
            self.step_dev.zero_()
            self.step_dev[0] = float(self.iterations)
        self.vel.copy_(sd["vel"])
        self.lr, self.momentum, self.decay, self.nesterov = sd["lr"], sd["momentum"], sd["decay"], sd["nesterov"]
        self.clipnorm, self.clipvalue = float(sd.get("clipnorm", 0.0)), float(sd.get("clipvalue", 0.0))


def make_optimizer(name: str, params, grads, **kw):
    name = name.lower()
    if name in ("adam", "adamw"):
        return FlatAdam(params, grads, **kw)
    if name in ("sgd", "sgd_nesterov"):
        return FlatSGD(params, grads, **kw)
    raise ValueError(f"unknown optimizer {name!r}")
