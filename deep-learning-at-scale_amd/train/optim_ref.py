"""Float64 references for the fused optimizer updates, with the error bounds beside them
(tests/test_optim_exact_*.py, tests/test_small_exact_gpu.py).

The update rules are written out by hand (no torch optimizer inside), in float64, on the exact
values the kernels are handed: fp32 tensors widened to float64 and hyperparameters rounded to
fp32 first (:func:`f32`), because that is what the launch receives. What then separates a
correct kernel from the reference is only the kernel's own fp32 roundings, and every bound
below is a count of those roundings read off the kernel text (csrc/elementwise.hip ``adam_one``,
``sgd_dev_kernel``; csrc/mlp_small.hip ``sb_adam``). ``U`` = 2^-24 is the unit roundoff of fp32: a
correctly rounded operation (``+ - * /``, ``sqrtf``, the IEEE division and square root hipcc emits
by default) errs by at most U relative, a 1-ulp hardware ``rcp`` / ``sqrt`` by at most 2 U.

One number cannot be derived: the error of ``__powf(b, t)`` in the bias corrections. It is
measured on the device (:data:`DELTA_POWF`, ``test_optim_exact_gpu.py::test_powf_error_is_within_delta``).
"""
from __future__ import annotations

import math

import torch

from .cnn_exact import keras_sgd_fp64

U = 2.0 ** -24
FLUSH = 2.0 ** -126   # a hardware exp2 result below this may be flushed to zero
SLACK = 1.001         # covers the products of two or more of the first-order terms below

# Relative error of the device's __powf(b, t) against float64 b^t: TWICE the worst value measured
# on an MI355X (1.68e-7) over b in {0.5, 0.9, 0.999} and every step number the tests reach (t = 1,
# 2, 3, 4, 10, 11, 12, 1000, 1001, 1002, 100000 ..), on the pairs with b^t >= 1/4, where the probe
# resolves delta to 1.5 U = 9e-8 or better (the measured worst includes that much of the probe's
# own rounding). For smaller b^t the probe holds the term the bound really contains,
# delta b^t / (1 - b^t), directly. test_optim_exact_gpu.py::test_powf_error_is_within_delta.
DELTA_POWF = 3.4e-7


def f32(x: float) -> float:
    """``x`` rounded to fp32 (what a ``(float)`` cast in the binding hands the kernel)."""
    return float(torch.tensor(float(x), dtype=torch.float32))


def is_pow2(x: float) -> bool:
    return x > 0 and math.frexp(x)[0] == 0.5


# ------------------------------------------------------------------------------ the gradient
def effective_grad_fp64(g: torch.Tensor, gscale: float = 1.0, clip_factor: float = 1.0,
                        clipvalue: float = 0.0) -> torch.Tensor:
    """``clamp(g * gscale * clip_factor, +-clipvalue)`` (clipvalue 0: no clamp), float64."""
    x = g.double() * gscale * clip_factor
    return x.clamp(-clipvalue, clipvalue) if clipvalue > 0 else x


def effective_grad_fp32(g: torch.Tensor, gscale: float, clip_factor: float | None, clipvalue: float) -> torch.Tensor:
    """The same value as the kernels form it (csrc/common.h clip_gscale, clip_grad): ``gs =
    fl(gscale * factor)`` (no product without a state block), ``x = fl(g * gs)``, the clamp."""
    gs = torch.tensor(gscale, dtype=torch.float32)
    if clip_factor is not None:
        gs = gs * torch.tensor(clip_factor, dtype=torch.float32)
    x = g.float() * gs
    return x.clamp(-clipvalue, clipvalue) if clipvalue > 0 else x


def grad_rel_error(gscale: float, clip_factor: float | None) -> float:
    """Relative error of :func:`effective_grad_fp32` against float64: 0 when the scale is a power
    of two (scaling is exact; a clamp only moves values onto the exact bound), else 2 U (the
    rounding of ``gs`` and of ``g * gs``)."""
    gs = f32(gscale) * (1.0 if clip_factor is None else f32(clip_factor))
    return 0.0 if is_pow2(gs) else 2 * U


# ------------------------------------------------------------------------------ Adam
def adam_fp64(p, g, m, v, t: int, lr: float, b1: float, b2: float, eps: float, wd: float = 0.0,
              gscale: float = 1.0, clip_factor: float = 1.0, clipvalue: float = 0.0):
    """One FlatAdam step (optim/flat.py), float64; ``t`` >= 1 is the number of this step.

    effective gradient ``ge = clamp(g * gscale * clip_factor, +-clipvalue)``;
    ``m' = b1 m + (1 - b1) ge``; ``v' = b2 v + (1 - b2) ge^2``;
    ``p' = p - lr (mh / (sqrt(vh) + eps) + wd p)``, ``mh = m' / (1 - b1^t)``, ``vh = v' / (1 - b2^t)``.
    Returns ``p', m', v'``."""
    p, m, v = p.double(), m.double(), v.double()
    ge = effective_grad_fp64(g, gscale, clip_factor, clipvalue)
    mn = b1 * m + (1.0 - b1) * ge
    vn = b2 * v + (1.0 - b2) * ge * ge
    mh = mn / (1.0 - b1 ** t)
    vh = vn / (1.0 - b2 ** t)
    pn = p - lr * (mh / (vh.sqrt() + eps) + wd * p)
    return pn, mn, vn


def adam_moments_fp32(g: torch.Tensor, b1: float, b2: float):
    """What fp32 must give for ``m`` and ``v`` after one step from zero state, bit for bit:
    ``m = fl(fl(1 - b1) * g)``, ``v = fl(fl(fl(1 - b2) * g) * g)`` (``g``: the effective gradient
    in fp32). The addend ``b m`` is zero, so fusing the multiply-add or not gives the same bits."""
    g = g.float()
    one = torch.tensor(1.0, dtype=torch.float32)
    c1 = one - torch.tensor(b1, dtype=torch.float32)
    c2 = one - torch.tensor(b2, dtype=torch.float32)
    return c1 * g, (c2 * g) * g


def adam_m_tol(g_eff, m, b1: float, g_rel: float = 0.0) -> torch.Tensor:
    """|m'_fp32 - m'_fp64| <= (3 U + g_rel) (b1 |m| + (1 - b1) |ge|).

    Roundings of ``m = b1 * m + (1.f - b1) * g``: ``1 - b1`` (U; exact for b1 >= 0.5), the product
    ``(1 - b1) g`` (U), the product ``b1 m`` (U, absent when the compiler fuses it into the add)
    and the sum (U of |m'| <= the bracket). Whichever of the two contractions is compiled, no
    term is charged more than 3 U."""
    s = b1 * m.double().abs() + (1.0 - b1) * g_eff.double().abs()
    return SLACK * (3 * U + g_rel) * s


def adam_v_tol(v_new, g_rel: float = 0.0) -> torch.Tensor:
    """|v'_fp32 - v'_fp64| <= (4 U + 2 g_rel) v'.

    Roundings of ``v = b2 * v + (1.f - b2) * g * g`` (left to right): ``1 - b2`` (U; exact for b2
    >= 0.5), ``(1 - b2) g`` (U), ``(..) g`` (U; absent when fused), ``b2 v`` (U; absent when fused),
    the sum (U). Every term is non-negative, so the bound is relative to v' itself: the g term
    carries at most 4 U, the v term at most 2 U."""
    return SLACK * (4 * U + 2 * g_rel) * v_new.double().abs()


# rounding counts (in U) of the two forms of the parameter update
_FORMS = {
    # adam_one: mh = m / bc1 (U), vh = v / bc2 (U), sqrtf (U), + eps (U), the division (U)
    "ieee": dict(mh=1, vh=1, sqrt=1, add=1, quot=1),
    # sb_adam: rbc = 1 / bc (U) then mh = m * rbc1 (U), vh = v * rbc2 (U); the hardware sqrt
    # (1 ulp = 2 U), + eps (U), the hardware rcp (2 U) and the product mh * rcp (U)
    "hw": dict(mh=2, vh=2, sqrt=2, add=1, quot=3),
}


def bias_correction_rel_error(b: float, t: int, delta: float) -> float:
    """Relative error of ``1.f - __powf(b, t)``: the pow's (``delta`` relative, or a flush of a
    result below 2^-126) over ``1 - b^t``, plus U for the subtraction."""
    x = b ** t
    return (delta * x + FLUSH) / (1.0 - x) + U


def adam_p_tol(p, g_eff, m, m_new, v_new, p_new, t: int, lr: float, b1: float, b2: float, eps: float, wd: float,
               delta: float = DELTA_POWF, form: str = "ieee", g_rel: float = 0.0) -> torch.Tensor:
    """|p'_fp32 - p'_fp64| for ``p -= lr * (mh / (sqrtf(vh) + eps) + wd * p)``; all arguments
    float64 reference values (``m``: the first moment BEFORE the step, for :func:`adam_m_tol`).

    With A = mh / (sqrt(vh) + eps) and X = A + wd p, first order:

    * m': :func:`adam_m_tol` absolute, divided by bc1 (sqrt(vh) + eps);
    * bc1: ``delta b1^t / (1 - b1^t)`` + U (:func:`bias_correction_rel_error`), relative to A;
    * bc2 the same and v' at most (4 U + 2 g_rel) relative, both HALVED by the square root;
    * the operations of the form (``_FORMS``): mh, vh (halved), sqrt, + eps, the quotient;
    * ``wd * p`` (U of |wd p|), the sum X (U of |X|), ``lr * X`` (U of |lr X|);
    * the final subtraction: U of |p'| (half an ulp).

    A fused multiply-add anywhere removes a rounding, never adds one. host-computed corrections
    (``adam_kernel``: bc1, bc2 arrive as rounded fp32 arguments) are covered with delta = 0."""
    k = _FORMS[form]
    p, g_eff, m, m_new, v_new, p_new = (x.double() for x in (p, g_eff, m, m_new, v_new, p_new))
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    den = (v_new / bc2).sqrt() + eps
    A = (m_new / bc1) / den
    rel = (bias_correction_rel_error(b1, t, delta) + k["mh"] * U
           + 0.5 * (bias_correction_rel_error(b2, t, delta) + (4 * U + 2 * g_rel) + k["vh"] * U)
           + (k["sqrt"] + k["add"] + k["quot"]) * U)
    err_a = A.abs() * rel + adam_m_tol(g_eff, m, b1, g_rel) / (bc1 * den)
    X = A + wd * p
    return SLACK * (lr * (err_a + U * (wd * p).abs() + 2 * U * X.abs()) + U * p_new.abs())


# ------------------------------------------------------------------------------ Keras-0.x SGD
def sgd_fp64(p, g, vel, it: int, lr: float, momentum: float, nesterov: bool, decay: float = 0.0,
             gscale: float = 1.0, clip_factor: float = 1.0, clipvalue: float = 0.0):
    """One FlatSGD step, float64: ``lr_t = lr / (1 + decay * it)`` around
    :func:`~wellflow.train.cnn_exact.keras_sgd_fp64` on the effective gradient. ``it`` >= 0 is
    the number of updates applied before this one. Returns ``p', vel'``."""
    ge = effective_grad_fp64(g, gscale, clip_factor, clipvalue)
    lr_t = lr / (1.0 + decay * it)
    return keras_sgd_fp64(p, ge, vel, lr_t, momentum, nesterov)


def sgd_tol(p_new, g_eff, vel, vel_new, it: int, lr: float, momentum: float, nesterov: bool, decay: float,
            g_rel: float = 0.0, host_lr: bool = False):
    """(|p' error|, |vel' error|) of ``sgd_dev_kernel`` / ``sgd_kernel``, float64 reference values in.

    ``lr_t = lr / (1.f + decay * it)``: the product, the sum and the division, 3 U relative (0 with
    decay = 0: ``lr / 1``; U when the host hands over a rounded fp32 ``lr_t``, ``host_lr``). With
    T = |lr_t ge|, whose product adds U (and g_rel):

    * ``v = momentum * vel - lr_t * gi``: U |momentum vel| + (k_lr + 1) U T + U |v'|;
    * Nesterov ``p += momentum * v - lr_t * gi``: momentum times the bound of v', the product
      ``momentum v`` (U), T again ((k_lr + 1) U), the inner sum (U) and the sum into p (U of |p'|);
    * plain momentum ``p += v``: the bound of v' and U of |p'|."""
    g_eff, vel, vel_new, p_new = (x.double() for x in (g_eff, vel, vel_new, p_new))
    k_lr = 1 if host_lr else (3 if decay != 0.0 else 0)
    lr_t = lr / (1.0 + decay * it)
    T = (lr_t * g_eff).abs()
    kt = (k_lr + 1) * U + g_rel
    e_v = U * (momentum * vel).abs() + kt * T + U * vel_new.abs()
    if nesterov:
        inner = momentum * vel_new - lr_t * g_eff
        e_p = momentum * e_v + U * (momentum * vel_new).abs() + kt * T + U * inner.abs() + U * p_new.abs()
    else:
        e_p = e_v + U * p_new.abs()
    return SLACK * e_p, SLACK * e_v
