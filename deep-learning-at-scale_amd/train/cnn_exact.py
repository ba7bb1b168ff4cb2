"""CNN training steps on data where bf16 / fp32 arithmetic is exact (tests/test_cnn_exact_*.py).

The recipe of train/exact.py, for the 1-D CNN of models/cnn.py: parameters, inputs and
per-element residuals are small dyadic numbers, so that

* every value a kernel rounds to bf16 (x, Wc with the conv bias, Wd, the pre-activations P,
  dOut * keep_scale, dAct; on the im2col + GEMM path also the stored ``act * keep_scale``, dpred
  and the masked dZc) needs at most 8 significant bits;
* every fp32 accumulation is a sum of multiples of one quantum, far below 2^24 quanta.

Nothing is ever rounded and no summation order matters, so a plain float64 step
(:func:`cnn_step_fp64`) must be matched BIT FOR BIT by the fused kernels (csrc/cnn_fused.hip), by
the im2col + GEMM path (csrc/gemm.hip, elementwise.hip) and by the small-batch kernel
(csrc/cnn_small.hip), wherever each places its roundings. :func:`cnn_exactness_violations` proves
the conditions for one problem, so a mismatch on the device can only be the kernel.

The lattice: Wc, Wd in {+-0.5, +-1} (dense, so every fragment slot holds a value a misplaced
slot would change), conv bias in {0, +-0.5, +-1}, dense bias in {0, +-0.5}, x in {-2 .. 2, step
0.5}, ``grad_scale`` a power of two <= 1/64 and <= 1 / (B * outputs), residuals e = pred - y in
{0, +-0.25, +-0.5, +-1} for MSE (dOut * keep_scale * Wd summed over 16 outputs keeps 8
significant bits) and in {0, +-0.25, +-0.5, +-1, +-2, 4} for clipped MAE with clip = 1 (on the
inclusive boundary, and beyond it).

Conventions (models/base.py ``per_element_loss`` + autograd, and every kernel): the dropout
mask is applied after ReLU; ``keep_scale`` = 1 / (1 - p) multiplies the dense output and dOut
(the GEMM path scales the stored activation and dZc instead: the same numbers on this data);
dP = dAct where the kept activation is nonzero; clipped MAE ``min(|d|, clip)`` with gradient
``sign(d) [|d| <= clip]`` (the boundary is inside), ``sign(0) = 0``; MSE ``d^2`` with gradient
``2 d``; ``d = pred - y``.

Also here: the bit-for-bit host mirror of the GEMM epilogue's dropout
(:func:`gemm_dropout_mask`), host encoders of the three bf16 operand images of the fused kernels
from their documented layout (:func:`cnn_images`), the float64 Keras SGD step
(:func:`keras_sgd_fp64`) and the comparator the tests share (:func:`block_mismatches`).

K-step launches of the small-batch kernel: after one update the parameters leave the lattice, so
two live steps cannot be exact. A launch in which ONE step has a nonzero gradient can: the other
batches are *dead* (clipped MAE, every residual far beyond the clip: loss B * outputs * clip, dOut
zero whatever the parameters) or *still* (MSE, targets = the prediction under that step's own
mask: everything zero, before the live step only). :func:`cnn_launch_fp64` replays such a launch,
:func:`cnn_launch_violations` proves it exact; the momentum then carries the live step's velocity
through the steps that follow, every intermediate an fp32 number.
"""
from __future__ import annotations

import dataclasses

import numpy as np
import torch

from ..models.cnn import CnnLayout
from .exact import MAX_QUANTA, _pick, _roundtrip_ok, _sum_ok, exact_grad_scale, quantum

W_VALUES = (-1.0, -0.5, 0.5, 1.0)
BC_VALUES = (-1.0, -0.5, 0.0, 0.5, 1.0)
BD_VALUES = (-0.5, 0.0, 0.5)
X_VALUES = (-2.0, -1.5, -1.0, -0.5, 0.0, 0.5, 1.0, 1.5, 2.0)
E_MSE = (-1.0, -0.5, -0.25, 0.0, 0.25, 0.5, 1.0)
E_MAE = (-2.0, -1.0, -0.5, -0.25, 0.0, 0.25, 0.5, 1.0, 2.0, 4.0)
CLIP = 1.0            # |e| = 1 sits on the (inclusive) boundary, |e| > 1 is cut


@dataclasses.dataclass
class CnnExactCase:
    lay: CnnLayout
    flat: torch.Tensor        # float64 [lay.numel], CnnLayout order (padding zero)
    x: torch.Tensor           # float64 [B][input_len][in_ch]
    e: torch.Tensor           # float64 [B][outputs]: the residual pred - y each element is given
    grad_scale: float         # a power of two
    loss: str
    dropout: float

    @property
    def keep_scale(self) -> float:
        return 1.0 / (1.0 - self.dropout) if self.dropout > 0 else 1.0


def cnn_grad_scale(B: int, outputs: int) -> float:
    """The power of two at or below 1 / (B * outputs), but no larger than 1 / 64."""
    return exact_grad_scale(B * outputs)


def exact_cnn_case(layout: CnnLayout, B: int, seed: int, loss: str = "mse", dropout: float = 0.0) -> CnnExactCase:
    """Parameters, inputs and residuals on the dyadic lattice (module docstring). From B = 16 on
    the middle window is all zeros: its pre-activations equal the conv bias, exactly 0 for a
    fifth of the filters, on top of the zeros the lattice produces by itself (about 3 %). The
    first four residuals are 0, the clip boundary (+1, -1) and one beyond it (within it for MSE)."""
    lay = layout
    g = torch.Generator(device="cpu").manual_seed(seed)
    flat = torch.zeros(lay.numel, dtype=torch.float64)
    Wc, Wd, bd = lay.views(flat)
    F, O = lay.filters, lay.outputs
    Wc[:F, : lay.taps] = _pick(W_VALUES, (F, lay.taps), g)
    Wc[:F, lay.taps] = _pick(BC_VALUES, (F,), g)
    Wd.view(lay.Op, lay.lout, lay.Fp)[:O, :, :F] = _pick(W_VALUES, (O, lay.lout, F), g)
    bd[:O] = _pick(BD_VALUES, (O,), g)
    x = _pick(X_VALUES, (B, lay.input_len, lay.in_ch), g)
    if B >= 16:
        x[B // 2] = 0.0
    e = _pick(E_MSE if loss == "mse" else E_MAE, (B, O), g)
    # the residuals every problem must hold: a zero, the clip boundary from both sides and one
    # beyond it (a problem of fewer than four elements gets one with a gradient instead)
    plant = (0.0, 1.0, 2.0 if loss == "mae_clip" else 0.5, -1.0)
    if B * O == len(plant) and loss == "mae_clip":
        # four elements in all: +1 and -1 would cancel in the dense-bias gradient (one output: the
        # sum of sign(e) over the batch), so the fourth is one within the clip
        plant = plant[:3] + (0.5,)
    if B * O >= len(plant):
        e.view(-1)[: len(plant)] = torch.tensor(plant, dtype=torch.float64)
    else:
        e.view(-1)[0] = -1.0
    return CnnExactCase(lay, flat, x, e, cnn_grad_scale(B, O), loss, float(dropout))


def _im2col(x: torch.Tensor, lay: CnnLayout) -> torch.Tensor:
    """[B][lout][taps], column k * in_ch + c = x[b][t + k][c] (csrc/elementwise.hip im2col1d_kernel)."""
    B = x.shape[0]
    return x.unfold(1, lay.kernel, 1).permute(0, 1, 3, 2).reshape(B, lay.lout, lay.taps)


def cnn_step_fp64(flat: torch.Tensor, x: torch.Tensor, y: torch.Tensor, grad_scale: float, loss: str = "mse",
                  clip: float = CLIP, mask: torch.Tensor | None = None, keep_scale: float = 1.0,
                  lay: CnnLayout = CnnLayout()) -> dict:
    """One training step in float64, forward and backward written out by hand (no autograd).

    ``flat`` in CnnLayout order, ``x`` [B][input_len][in_ch] (or [B][input_len] for one channel),
    ``y`` [B][outputs], ``mask`` the keep mask [B][lout][Fp] (bool; None = keep everything).
    Returns, all in the padded layout with the padding zero: ``pred``, ``per``, ``dout``
    [B][Op], ``loss_sum`` (0-dim), ``grads`` (flat) and the intermediates ``P`` (pre-activations),
    ``act`` (ReLU, then the mask; unscaled), ``dAct`` (= keep_scale * dOut Wd) and ``dP``, each
    [B][lout][Fp]."""
    flat, x, y = flat.double(), x.double(), y.double()
    B = x.shape[0]
    x = x.reshape(B, lay.input_len, lay.in_ch)
    O, Op, T, Fp, taps = lay.outputs, lay.Op, lay.lout, lay.Fp, lay.taps
    Wc, Wd, bd = lay.views(flat)
    cols = _im2col(x, lay)
    P = cols @ Wc[:, :taps].t() + Wc[:, taps]                     # [B][T][Fp]
    act = torch.where(P > 0, P, torch.zeros_like(P))
    if mask is not None:
        act = act * mask.reshape(B, T, Fp).double()
    h = act.reshape(B, T * Fp)
    pred = keep_scale * (h @ Wd.t()) + bd                          # [B][Op]
    ypad = torch.zeros(B, Op, dtype=torch.float64)
    ypad[:, :O] = y.reshape(B, O)
    live = torch.zeros(B, Op, dtype=torch.float64)
    live[:, :O] = 1.0
    d = (pred - ypad) * live
    if loss == "mse":
        per, dout = d * d, 2.0 * grad_scale * d
    elif loss == "mae_clip":
        per = d.abs().clamp(max=clip)
        dout = grad_scale * torch.sign(d) * (d.abs() <= clip).double()
    else:
        raise ValueError(f"unknown loss {loss!r}")
    ds = dout * keep_scale
    grads = torch.zeros(lay.numel, dtype=torch.float64)
    gWc, gWd, gbd = lay.views(grads)
    gWd.copy_(ds.t() @ h)
    gbd.copy_(dout.sum(0))
    dAct = (ds @ Wd).reshape(B, T, Fp)
    dP = dAct * (act != 0).double()
    gWc[:, :taps] = dP.reshape(B * T, Fp).t() @ cols.reshape(B * T, taps)
    gWc[:, taps] = dP.sum((0, 1))
    return {"pred": pred, "per": per, "loss_sum": per.sum(), "dout": dout, "grads": grads,
            "P": P, "act": act, "dAct": dAct, "dP": dP}


def cnn_forward_fp64(flat: torch.Tensor, x: torch.Tensor, lay: CnnLayout) -> torch.Tensor:
    """The evaluation forward in float64: predictions [B][Op], no mask and no keep scale."""
    B = x.shape[0]
    Wc, Wd, bd = lay.views(flat.double())
    cols = _im2col(x.double().reshape(B, lay.input_len, lay.in_ch), lay)
    P = cols @ Wc[:, : lay.taps].t() + Wc[:, lay.taps]
    return torch.where(P > 0, P, torch.zeros_like(P)).reshape(B, -1) @ Wd.t() + bd


def exact_cnn_targets(case: CnnExactCase, mask: torch.Tensor | None) -> torch.Tensor:
    """y = pred - e (float64 [B][outputs]): the targets that give each element its residual."""
    B, O = case.e.shape
    ref = cnn_step_fp64(case.flat, case.x, torch.zeros(B, O, dtype=torch.float64), 0.0, "mse", CLIP, mask,
                        case.keep_scale, case.lay)
    return ref["pred"][:, :O] - case.e


# ------------------------------------------------------------------------- dropout mirrors
_M64 = (1 << 64) - 1


def seed32(seed: int) -> int:
    """models/cnn.py NativeCNN.seed32: the 31-bit kernel seed of an engine seed."""
    return (seed * 1000003) & 0x7FFFFFFF


def gemm_dropout_mask(seed: int, step: int | None, M: int, N: int, p: float) -> torch.Tensor:
    """Keep mask [M][N] (bool) of the GEMM epilogue's dropout, bit for bit:
    ``uniform_hash(drop_seed(e), m * N + n) >= p`` with csrc/common.h uniform_hash (splitmix64
    finaliser of seed + idx * 0x9E3779B97F4A7C15, top 24 bits as an fp32 in [0, 1)) and
    csrc/gemm.hip drop_seed (seed ^ step * 0xD1B54A32D192ED03, all modulo 2^64). ``step`` is the
    device step counter the launch reads (NativeCNN.rng before the step); None = no counter."""
    s = seed & _M64
    if step is not None:
        s ^= ((step & _M64) * 0xD1B54A32D192ED03) & _M64
    u = uniform_hash(s, np.arange(M * N, dtype=np.uint64))
    return torch.from_numpy(u >= np.float32(p)).reshape(M, N)


def uniform_hash(seed: int, idx: np.ndarray) -> np.ndarray:
    """csrc/common.h uniform_hash over a uint64 index array: fp32 values in [0, 1), every
    product and sum modulo 2^64."""
    with np.errstate(over="ignore"):
        z = np.uint64(seed & _M64) + idx.astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(40)).astype(np.float32) * np.float32(1.0 / 16777216.0)


# ---------------------------------------------------------------------- the operand images
def cnn_images(flat: torch.Tensor, lay: CnnLayout) -> dict:
    """The three bf16 operand images of the fused kernels, written from the layout documented
    in csrc/cnn_fused.hip (cnn_pack_kernel), as float64 tensors of the values:

    * ``WcA`` [Fp * Kc]: the conv block as it is (the bias in column taps);
    * ``WdB`` [T][7 blocks][64 lanes][4]: lane 16 q + l holds Wd[4 q + jj][t Fp + 16 b + l];
    * ``WdF``: per step three interleaved block pairs [64 lanes][8] (lane 16 q + j: block 2 p's
      Wd[j][t Fp + 32 p + 4 q + jj] in its first four slots, block 2 p + 1's in the next four),
      then block 6 as [64 lanes][4];

    rows j >= outputs of the dense block are ZERO in both dense images whatever ``flat`` holds."""
    Wc, Wd, _ = lay.views(flat.double())
    T, Fp, NFB = lay.lout, lay.Fp, lay.Fp // 16
    W = Wd.reshape(16, T, Fp).clone()
    W[lay.outputs:] = 0.0
    WdB = W.reshape(4, 4, T, NFB, 16).permute(2, 3, 0, 4, 1).reshape(T, NFB, 64, 4)       # [t][b][q, l][jj]
    FB = W.reshape(16, T, NFB, 4, 4).permute(1, 2, 3, 0, 4).reshape(T, NFB, 64, 4)        # [t][b][q, j][jj]
    pairs = [torch.stack((FB[:, 2 * p], FB[:, 2 * p + 1]), dim=2).reshape(T, 512) for p in range(NFB // 2)]
    tail = [FB[:, b].reshape(T, 256) for b in range(2 * (NFB // 2), NFB)]
    WdF = torch.cat(pairs + tail, dim=1)
    return {"WcA": Wc.reshape(-1).clone(), "WdF": WdF.reshape(-1).contiguous(), "WdB": WdB.reshape(-1).contiguous()}


def keras_sgd_fp64(p: torch.Tensor, g: torch.Tensor, v: torch.Tensor, lr: float, momentum: float, nesterov: bool,
                   decay: float = 0.0, iteration: int = 0):
    """One Keras-0.x SGD step in float64 (optim/flat.py FlatSGD): returns (params, velocities)."""
    lr_t = lr / (1.0 + decay * iteration)
    vn = momentum * v.double() - lr_t * g.double()
    pn = p.double() + (momentum * vn - lr_t * g.double() if nesterov else vn)
    return pn, vn


# --------------------------------------------------------------------------------- the proof
def cnn_exactness_violations(case: CnnExactCase, y: torch.Tensor, mask: torch.Tensor | None, path: str = "fused",
                             clip: float = CLIP, sgd: dict | None = None) -> list:
    """Why a kernel could legitimately differ from :func:`cnn_step_fp64` on this problem: an
    empty list when

    (a) everything a path rounds to bf16 survives the round trip: x, Wc with the conv bias (an
        MFMA K slot against a constant 1), Wd, P, dOut * keep_scale and dAct; for ``path`` =
        "gemm" also the stored activation ``act * keep_scale`` (Hc), dpred and dZc = dP;
    (b) everything held in fp32 survives its round trip: the parameters, y, pred, pred - y, the
        per-element loss, dOut, the loss sum and every gradient block; the evaluation forward's
        predictions (no mask, no keep scale) as well;
    (c) for every accumulation (each pre-activation, each dense output with and without the mask,
        dAct, dWd, dWc with its bias row, the dense-bias gradient, the loss sum) the sum of
        |terms| stays below 2^24 quanta of its terms, so any partial sum in any order is an fp32
        number;
    (d) with ``sgd`` = {"lr", "momentum", "nesterov"} and optionally {"decay", "iteration",
        "velocities"} (the small-batch kernel, which applies the Keras update itself; zero decay,
        counter and velocities unless given): :func:`sgd_update_violations` finds nothing."""
    bad: list = []
    lay, ks = case.lay, case.keep_scale
    B = case.x.shape[0]
    O, T, Fp, taps = lay.outputs, lay.lout, lay.Fp, lay.taps
    ref = cnn_step_fp64(case.flat, case.x, y, case.grad_scale, case.loss, clip, mask, ks, lay)
    Wc, Wd, bd = lay.views(case.flat)
    bf, f32 = torch.bfloat16, torch.float32
    P, act, dAct, dP, dout = ref["P"], ref["act"], ref["dAct"], ref["dP"], ref["dout"]
    ds = dout * ks
    _roundtrip_ok("x", case.x, bf, bad)
    _roundtrip_ok("Wc with the conv bias", Wc, bf, bad)
    _roundtrip_ok("Wd", Wd, bf, bad)
    _roundtrip_ok("P", P, bf, bad)
    _roundtrip_ok("dOut * keep_scale", ds, bf, bad)
    _roundtrip_ok("dAct", dAct, bf, bad)
    if path == "gemm":
        _roundtrip_ok("Hc = act * keep_scale", act * ks, bf, bad)
        _roundtrip_ok("dpred", dout, bf, bad)
        _roundtrip_ok("dZc", dP, bf, bad)
    pred_eval = cnn_forward_fp64(case.flat, case.x, lay)
    ypad = torch.zeros(B, lay.Op, dtype=torch.float64)
    ypad[:, :O] = y
    for name, t in (("flat params", case.flat), ("y", y), ("pred", ref["pred"]), ("pred - y", ref["pred"] - ypad),
                    ("per", ref["per"]), ("dOut", dout), ("loss_sum", ref["loss_sum"]), ("pred (eval)", pred_eval),
                    ("act", act), ("dAct (fp32)", dAct)):
        _roundtrip_ok(name, t, f32, bad)
    gWc, gWd, gbd = lay.views(ref["grads"])
    for name, t in (("gWc", gWc), ("gWd", gWd), ("gbd", gbd)):
        _roundtrip_ok(name, t, f32, bad)
    # accumulations; a product's quantum is (at least) the product of its factors' quanta
    cols = _im2col(case.x, lay).abs()
    Wt, bc = Wc[:, :taps], Wc[:, taps]
    qx, qWc, qWd = quantum(case.x), quantum(Wt), quantum(Wd)
    _sum_ok("P", cols @ Wt.abs().t() + bc.abs(), min(qx * qWc, quantum(bc)), bad)
    reluP = torch.where(P > 0, P, torch.zeros_like(P))
    qa = quantum(reluP)
    for name, a, s in (("pred", act, ks), ("pred (eval)", reluP, 1.0)):
        _sum_ok(name, s * (a.reshape(B, -1).abs() @ Wd.abs().t()) + bd.abs(), min(s * qa * qWd, quantum(bd)), bad)
    qd = quantum(ds)
    _sum_ok("dAct", ds.abs() @ Wd.abs(), min(qd, quantum(dout)) * qWd, bad)
    _sum_ok("gWd", ds.abs().t() @ act.reshape(B, -1).abs(), min(qd, quantum(dout)) * qa, bad)
    qp = quantum(dP)
    _sum_ok("gWc", dP.reshape(B * T, Fp).abs().t() @ cols.reshape(B * T, taps), qp * qx, bad)
    _sum_ok("gWc bias row", dP.abs().sum((0, 1)), qp, bad)
    _sum_ok("gbd", dout.abs().sum(0), quantum(dout), bad)
    _sum_ok("loss_sum", ref["per"].abs().sum().reshape(1), quantum(ref["per"]), bad)
    if sgd is not None:
        vel = sgd.get("velocities")
        vel = torch.zeros_like(ref["grads"]) if vel is None else vel
        sgd_update_violations(case.flat, ref["grads"], vel, sgd, sgd.get("iteration", 0), bad)
    return bad


def sgd_lr_t_fp32(lr: float, decay: float, iteration: float) -> float:
    """``lr / (1.f + decay * it)`` as the small kernel forms it: three fp32 operations on fp32 values."""
    t = lambda v: torch.tensor(float(v), dtype=torch.float32)  # noqa: E731
    return float(t(lr) / (t(1.0) + t(decay) * t(iteration)))


def sgd_update_violations(p: torch.Tensor, g: torch.Tensor, v: torch.Tensor, sgd: dict, iteration: int, bad: list,
                          tag: str = "") -> None:
    """Condition (d) of :func:`cnn_exactness_violations` for one Keras step from parameters ``p``,
    gradient ``g`` and velocities ``v`` (float64) at step counter ``iteration``: with a nonzero
    gradient the kernel's fp32 ``lr_t`` is the float64 one; ``momentum * v``, ``lr_t * g``, the new
    velocities, ``momentum * v'``, the Nesterov sum and the new parameters are fp32 numbers (so
    each operation's exact result is representable, fused into a multiply-add or not) and the
    update sums fewer than 2^24 quanta."""
    f32 = torch.float32
    lr, mu, decay = sgd["lr"], sgd["momentum"], sgd.get("decay", 0.0)
    lr_t = lr / (1.0 + decay * iteration)
    if bool((g != 0).any()) and sgd_lr_t_fp32(lr, decay, iteration) != lr_t:
        bad.append(f"{tag}lr_t: fp32 gives {sgd_lr_t_fp32(lr, decay, iteration)!r}, float64 {lr_t!r}")
    pn, vn = keras_sgd_fp64(p, g, v, lr, mu, sgd["nesterov"], decay, iteration)
    for name, t in (("momentum * v", mu * v), ("lr * g", lr_t * g), ("new velocities", vn), ("momentum * v'", mu * vn),
                    ("momentum * v' - lr * g", mu * vn - lr_t * g), ("new parameters", pn)):
        _roundtrip_ok(tag + name, t, f32, bad)
    terms = p.abs() + (mu + 1.0) * (mu * v.abs() + lr_t * g.abs())
    q = min(quantum(p), mu * lr_t * quantum(g), mu * mu * quantum(v))
    _sum_ok(tag + "SGD update", terms, q, bad)


# ------------------------------------------------------------------- K-step launches, replayed
DEAD_OFFSET = 64.0    # a dead batch's targets: the float64 prediction +- this (far beyond CLIP)
DEAD_MARGIN = 32.0    # every |pred - y| of a dead step must stay above this in the replay
VEL_VALUES = (-0.5, -0.375, -0.25, -0.125, 0.0, 0.125, 0.25, 0.375, 0.5)


def lattice_velocities(lay: CnnLayout, seed: int) -> torch.Tensor:
    """Velocities on the lattice (multiples of 1/8 in [-0.5, 0.5]) for every live parameter, zero
    on all padding: float64 [lay.numel]."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    flat = torch.zeros(lay.numel, dtype=torch.float64)
    Wc, Wd, bd = lay.views(flat)
    F, O = lay.filters, lay.outputs
    Wc[:F, : lay.taps + 1] = _pick(VEL_VALUES, (F, lay.taps + 1), g)
    Wd.view(lay.Op, lay.lout, lay.Fp)[:O, :, :F] = _pick(VEL_VALUES, (O, lay.lout, F), g)
    bd[:O] = _pick(VEL_VALUES, (O,), g)
    return flat


def _train_pred(flat, x, mask, keep_scale, lay) -> torch.Tensor:
    B = x.shape[0]
    zero = torch.zeros(B, lay.outputs, dtype=torch.float64)
    return cnn_step_fp64(flat, x, zero, 0.0, "mse", CLIP, mask, keep_scale, lay)["pred"][:, : lay.outputs]


def still_targets(flat, x, mask, keep_scale: float, lay: CnnLayout) -> torch.Tensor:
    """Targets of a *still* MSE batch: the float64 training prediction under this step's own mask,
    so every residual, the loss and every gradient are exactly 0 (while ``flat`` is what the step
    starts from; under any other mask the step is live)."""
    return _train_pred(flat, x, mask, keep_scale, lay)


def dead_targets(flat, x, mask, keep_scale: float, lay: CnnLayout, seed: int) -> torch.Tensor:
    """Targets of a *dead* clipped-MAE batch: the float64 prediction from ``flat`` (the parameters
    the step starts from, on the lattice or not) +- DEAD_OFFSET, signs drawn from ``seed``,
    rounded to fp32. Every residual is far beyond the clip, so the loss sum is B * outputs * clip
    and dOut is zero however the kernel rounds its prediction."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    pred = _train_pred(flat, x, mask, keep_scale, lay)
    return (pred + DEAD_OFFSET * _pick((-1.0, 1.0), tuple(pred.shape), g)).float().double()


def cnn_launch_fp64(flat: torch.Tensor, vel: torch.Tensor, steps, grad_scale: float, loss: str, clip: float,
                    keep_scale: float, lay: CnnLayout, sgd: dict, it0: int = 0) -> dict:
    """A K-step launch of the small-batch kernel replayed in float64. ``steps``: K tuples (x, y,
    mask), the mask being that of device step ``rng0 + k`` (None without dropout). Step k is
    :func:`cnn_step_fp64` on batch k from the current parameters, then :func:`keras_sgd_fp64` with
    ``iteration = it0 + k`` (``sgd``: lr, momentum, nesterov, decay). Returns ``params``,
    ``velocities``, ``loss_sum`` (summed over the steps) and ``trace``: per step the state it
    started from (``params``, ``velocities``), its ``ref`` (the cnn_step_fp64 dict) and ``loss``."""
    p, v = flat.double().clone(), vel.double().clone()
    total = torch.zeros((), dtype=torch.float64)
    trace = []
    for k, (x, y, mask) in enumerate(steps):
        ref = cnn_step_fp64(p, x, y, grad_scale, loss, clip, mask, keep_scale, lay)
        trace.append({"params": p, "velocities": v, "ref": ref, "loss": ref["loss_sum"]})
        p, v = keras_sgd_fp64(p, ref["grads"], v, sgd["lr"], sgd["momentum"], sgd["nesterov"], sgd.get("decay", 0.0),
                              it0 + k)
        total = total + ref["loss_sum"]
    return {"params": p, "velocities": v, "loss_sum": total, "trace": trace}


def cnn_launch_violations(case: CnnExactCase, vel: torch.Tensor, steps, kinds, sgd: dict, it0: int, clip: float = CLIP,
                          loss0: float = 0.0) -> list:
    """Why the small-batch kernel could legitimately differ from :func:`cnn_launch_fp64` on a
    launch with ONE live step (``kinds``: "live", "dead" or "still" per step; ``case`` holds the
    parameters, grad_scale, loss and dropout; the live batch is steps[k_live]). Empty when

    * every step up to the live one, and every still step, starts from ``case.flat`` and passes
      :func:`cnn_exactness_violations` (the live one with its Keras update from the velocities and
      step counter it meets);
    * every still step has residuals, loss and gradients exactly 0; every dead step has all
      |pred - y| > DEAD_MARGIN (a clipped-MAE launch), loss B * outputs * clip and zero gradients;
    * every step's update passes :func:`sgd_update_violations` (so every intermediate parameter
      and velocity is an fp32 number), every target is one, and the loss accumulated from
      ``loss0`` is one after every step."""
    bad: list = []
    lay, ks = case.lay, case.keep_scale
    if list(kinds).count("live") != 1:
        return [f"kinds {kinds}: exactly one live step expected"]
    k_live = list(kinds).index("live")
    run = cnn_launch_fp64(case.flat, vel, steps, case.grad_scale, case.loss, clip, ks, lay, sgd, it0)
    acc = float(loss0)
    for k, ((x, y, mask), kind, tr) in enumerate(zip(steps, kinds, run["trace"])):
        tag = f"step {k} ({kind}): "
        ref = tr["ref"]
        B = x.shape[0]
        _roundtrip_ok(tag + "y", y, torch.float32, bad)
        if k <= k_live or kind == "still":
            if not torch.equal(tr["params"], case.flat.double()):
                bad.append(tag + "does not start from the lattice parameters")
            ck = CnnExactCase(lay, tr["params"], x, case.e, case.grad_scale, case.loss, case.dropout)
            live_sgd = dict(sgd, velocities=tr["velocities"], iteration=it0 + k) if kind == "live" else None
            bad += [tag + v for v in cnn_exactness_violations(ck, y, mask, "small", clip, live_sgd)]
        d = ref["pred"][:, : lay.outputs] - y
        if kind == "still":
            if case.loss != "mse" or bool((d != 0).any()) or float(ref["loss_sum"]) != 0.0:
                bad.append(tag + "a residual is not 0")
        if kind == "dead":
            if case.loss != "mae_clip" or not float(d.abs().min()) > max(DEAD_MARGIN, 2 * clip):
                bad.append(tag + f"a residual within {DEAD_MARGIN} of the clip")
            if float(ref["loss_sum"]) != B * lay.outputs * clip:
                bad.append(tag + f"loss {float(ref['loss_sum'])!r} is not B * outputs * clip")
        if kind != "live" and bool((ref["grads"] != 0).any()):
            bad.append(tag + "a gradient is not 0")
        if kind == "live" and not all(bool((b != 0).any()) for b in lay.views(ref["grads"])):
            bad.append(tag + "a gradient block of the live step is all zero")
        sgd_update_violations(tr["params"], ref["grads"], tr["velocities"], sgd, it0 + k, bad, tag)
        acc += float(ref["loss_sum"])
        if float(torch.tensor(acc, dtype=torch.float32)) != acc:
            bad.append(tag + f"accumulated loss {acc!r} is no fp32 number")
    for name in ("params", "velocities"):
        _roundtrip_ok(f"final {name}", run[name], torch.float32, bad)
    return bad


# ---------------------------------------------------------------------------- the comparator
def block_mismatches(got: dict, want: dict) -> list:
    """``torch.equal`` of every named block of ``want`` (cast by the caller) against ``got``;
    one line per differing block: its name, how many elements differ, the first differing flat
    index and both values there. The tests assert that the list is empty."""
    bad = []
    for name, w in want.items():
        g = got[name]
        if g.shape != w.shape or g.dtype != w.dtype:
            bad.append(f"{name}: shape / dtype {tuple(g.shape)} {g.dtype} != {tuple(w.shape)} {w.dtype}")
            continue
        if torch.equal(g, w):
            continue
        ne = (g != w).reshape(-1)
        i = int(ne.nonzero()[0])
        bad.append(f"{name}: {int(ne.sum())} of {w.numel()} differ, first at flat index {i}: got "
                   f"{float(g.reshape(-1)[i])!r}, want {float(w.reshape(-1)[i])!r}")
    return bad


def step_blocks(ref: dict, lay: CnnLayout, mult: float = 1.0) -> dict:
    """The float64 reference of one step as the fp32 blocks the GPU tests compare: ``dout``
    [B][16], ``loss``, ``gWc`` (bias column and padding included), ``gWd``, ``gbd``."""
    gWc, gWd, gbd = lay.views((ref["grads"] * mult).float())
    return {"dout": ref["dout"].float(), "loss": ref["loss_sum"].reshape(1).float(), "gWc": gWc, "gWd": gWd, "gbd": gbd}


__all__ = ["CLIP", "DEAD_MARGIN", "DEAD_OFFSET", "MAX_QUANTA", "CnnExactCase", "block_mismatches",
           "cnn_exactness_violations", "cnn_forward_fp64", "cnn_grad_scale", "cnn_images", "cnn_launch_fp64",
           "cnn_launch_violations", "cnn_step_fp64", "dead_targets", "exact_cnn_case", "exact_cnn_targets",
           "gemm_dropout_mask", "keras_sgd_fp64", "lattice_velocities", "seed32", "sgd_lr_t_fp32", "sgd_update_violations",
           "step_blocks", "still_targets", "uniform_hash"]
