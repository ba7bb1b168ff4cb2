"""MLP training steps on data where bf16 / fp32 arithmetic is exact (tests/test_mlp_exact_*.py).

Random data cannot anchor the MLP kernels more sharply than ~3e-2 per gradient block: rounding
H1 to bf16 moves the layer-2 pre-activations by ~1e-2 of their spread, about 0.1 % of the ReLU
masks flip against a float64 step, and every flip is a full-size error in dZ2. So the tests
choose the weights as well as the inputs, all small dyadic numbers:

* every value a kernel rounds to bf16 (X, W, H_l, dZ_l) needs at most 8 significant bits;
* every fp32 accumulation is a sum of multiples of one quantum, far below 2^24 quanta.

Nothing is ever rounded, the summation order does not matter, and a ReLU pre-activation is
either exactly 0 or a whole quantum away from 0. A plain float64 step of the same operation
(:func:`mlp_step_fp64`) must then be matched BIT FOR BIT by every kernel path, wherever it
places its roundings. :func:`exactness_violations` proves the two conditions for a case, so a
mismatch on the device can only be the kernel.

Conventions (shared by models/base.py ``per_element_loss`` + autograd and by every kernel):
ReLU mask ``H > 0``; clipped MAE ``min(|d|, clip)`` with gradient ``sign(d) [|d| <= clip]``
(the boundary is inside), ``sign(0) = 0``; MSE ``d^2`` with gradient ``2 d``; ``d = pred - y``.
"""
from __future__ import annotations

import dataclasses

import torch

from ..models.mlp import MlpLayout

W_VALUES = (-1.0, -0.5, 0.5, 1.0)
B1_VALUES = (-1.0, -0.5, 0.0, 0.5, 1.0)
BL_VALUES = (-2.0, -1.5, -1.0, -0.5, 0.0, 0.5, 1.0)          # biases of the layers after the first
X_VALUES = (-2.0, -1.5, -1.0, -0.5, 0.0, 0.5, 1.0, 1.5, 2.0)
E_VALUES = (-2.0, -1.0, -0.5, -0.25, 0.0, 0.25, 0.5, 1.0, 2.0, 4.0)  # pred - y per row
B_HEAD = 0.5
CLIP = 1.0            # |e| = 1 rows sit on the (inclusive) boundary, |e| > 1 rows are cut
NNZ = 4               # nonzeros per weight row
MAX_QUANTA = 1 << 24  # fp32 holds every integer multiple of a quantum below this


@dataclasses.dataclass
class ExactCase:
    lay: MlpLayout
    flat: torch.Tensor        # float64 [lay.numel], MlpLayout order (padding columns zero)
    x: torch.Tensor           # float64 [B][F]
    e: torch.Tensor           # float64 [B]: the residual pred - y each row is given
    grad_scale: float         # a power of two


def _pick(values, shape, g) -> torch.Tensor:
    v = torch.tensor(values, dtype=torch.float64)
    return v[torch.randint(0, len(values), shape, generator=g)]


def exact_grad_scale(B: int) -> float:
    """The power of two at or below 1 / B, but no larger than 1 / 64."""
    s = 1.0 / 64
    while s * B > 1.0:
        s /= 2
    return s


def exact_mlp_case(F: int, hidden, B: int, seed: int) -> ExactCase:
    """Weights, inputs and residuals on the dyadic lattice (module docstring). Weight rows hold
    ``min(4, fan_in)`` nonzeros from {+-0.5, +-1} at random columns; about 10 % of the head
    weights are 0. ``grad_scale`` is 1/64 up to B = 64, 1/256 at 192, 1/512 at 300."""
    hidden = tuple(hidden)
    lay = MlpLayout(F, hidden)
    g = torch.Generator(device="cpu").manual_seed(seed)
    flat = torch.zeros(lay.numel, dtype=torch.float64)
    layers, hw, hb = lay.views(flat)
    fan = F
    for l, (W, b) in enumerate(layers):
        h = W.shape[0]
        n = min(NNZ, fan)
        cols = torch.rand(h, fan, generator=g).argsort(dim=1)[:, :n]
        W.scatter_(1, cols, _pick(W_VALUES, (h, n), g))
        b.copy_(_pick(B1_VALUES if l == 0 else BL_VALUES, (h,), g))
        fan = h
    w3 = _pick(W_VALUES, (fan,), g)
    w3[torch.rand(fan, generator=g) < 0.1] = 0.0
    hw.copy_(w3)
    hb.fill_(B_HEAD)
    x = _pick(X_VALUES, (B, F), g)
    e = _pick(E_VALUES, (B,), g)
    return ExactCase(lay, flat, x, e, exact_grad_scale(B))


def exact_targets(case: ExactCase) -> torch.Tensor:
    """y = pred - e (float64): the targets that give row b the residual ``e[b]``."""
    y0 = torch.zeros(case.x.shape[0], dtype=torch.float64)
    return mlp_step_fp64(case.flat, case.x, y0, 0.0, "mse", CLIP, hidden=case.lay.hidden)["pred"] - case.e


def mlp_step_fp64(flat: torch.Tensor, x: torch.Tensor, y: torch.Tensor, grad_scale: float,
                  loss: str = "mse", clip: float = CLIP, hidden=(256, 256)) -> dict:
    """One training step in float64, forward and backward written out by hand.

    ``flat`` in MlpLayout order for ``x.shape[1]`` features and ``hidden``; returns ``pred``
    [B], ``loss_sum`` (0-dim), ``grads`` (flat, MlpLayout order, padding zero), and the
    intermediates ``Z`` (pre-activations), ``H`` (activations, H[0] = x), ``dZ`` per layer and
    ``dy`` = grad_scale * dLoss/dpred."""
    x, y = x.double(), y.double()
    B, F = x.shape
    lay = MlpLayout(F, tuple(hidden))
    layers, hw, hb = lay.views(flat.double())
    H, Z = [x], []
    for W, b in layers:
        z = H[-1] @ W[:, : H[-1].shape[1]].t() + b
        Z.append(z)
        H.append(torch.where(z > 0, z, torch.zeros_like(z)))
    pred = H[-1] @ hw + hb
    d = pred - y
    if loss == "mse":
        per, dy = d * d, 2.0 * grad_scale * d
    elif loss == "mae_clip":
        per = d.abs().clamp(max=clip)
        dy = grad_scale * torch.sign(d) * (d.abs() <= clip).double()
    else:
        raise ValueError(f"unknown loss {loss!r}")
    grads = torch.zeros(lay.numel, dtype=torch.float64)
    glayers, ghw, ghb = lay.views(grads)
    ghw.copy_(H[-1].t() @ dy)
    ghb.copy_(dy.sum().reshape(1))
    dZ = [None] * len(layers)
    dH = dy[:, None] * hw[None, :]
    for l in range(len(layers) - 1, -1, -1):
        dz = dH * (H[l + 1] > 0).double()
        dZ[l] = dz
        gW, gb = glayers[l]
        gW[:, : H[l].shape[1]].copy_(dz.t() @ H[l])
        gb.copy_(dz.sum(0))
        if l > 0:
            dH = dz @ layers[l][0]
    return {"pred": pred, "loss_sum": per.sum(), "grads": grads, "Z": Z, "H": H, "dZ": dZ, "dy": dy, "per": per}


def quantum(t: torch.Tensor) -> float:
    """The largest power of two that divides every element of ``t`` (1.0 for all zeros)."""
    t = t.double().reshape(-1)
    t = t[t != 0]
    if t.numel() == 0:
        return 1.0
    q = 2.0 ** 40
    while not bool(((t / q) == (t / q).round()).all()):
        q /= 2
        if q < 2.0 ** -80:
            raise ValueError("not dyadic")
    return q


def _sum_ok(name: str, abs_sum: torch.Tensor, q: float, bad: list) -> None:
    # abs_sum: per output element, the sum of |terms| of its accumulation; q: a quantum of every term
    n = float(abs_sum.max()) / q if abs_sum.numel() else 0.0
    if not n < MAX_QUANTA:
        bad.append(f"{name}: {n:.3g} quanta of {q:g} >= 2^24")


def _roundtrip_ok(name: str, t: torch.Tensor, dtype, bad: list) -> None:
    if not torch.equal(t.to(dtype).double(), t.double()):
        i = int((t.to(dtype).double() != t.double()).reshape(-1).nonzero()[0])
        bad.append(f"{name}: not exact in {dtype} (first at {i}: {float(t.reshape(-1)[i])!r})")


def exactness_violations(case: ExactCase, y: torch.Tensor, loss: str, clip: float = CLIP) -> list:
    """Why a kernel could legitimately differ from :func:`mlp_step_fp64` on this case: an empty
    list when (a) X, every W, H_l and dZ_l survive a bf16 round trip, (b) y, pred, the
    per-row loss, dy, the loss sum and every gradient block survive an fp32 round trip and (c)
    for every accumulation (each pre-activation, the head, dH_l = dZ_{l+1} W_{l+1}, each weight /
    bias / head gradient, the loss sum) the sum of |terms| stays below 2^24 quanta of its terms,
    so that any partial sum in any order is an fp32 number."""
    bad: list = []
    lay = case.lay
    ref = mlp_step_fp64(case.flat, case.x, y, case.grad_scale, loss, clip, hidden=lay.hidden)
    layers, hw, hb = lay.views(case.flat)
    bf, f32 = torch.bfloat16, torch.float32
    _roundtrip_ok("x", case.x, bf, bad)
    _roundtrip_ok("flat params (fp32)", case.flat, f32, bad)
    for l, (W, b) in enumerate(layers):
        _roundtrip_ok(f"W{l + 1}", W, bf, bad)
        _roundtrip_ok(f"b{l + 1} (folded into the MFMA accumulator by the 128-row step)", b, bf, bad)
        _roundtrip_ok(f"H{l + 1}", ref["H"][l + 1], bf, bad)
        _roundtrip_ok(f"dZ{l + 1}", ref["dZ"][l], bf, bad)
    for name in ("pred", "loss_sum", "dy", "per"):
        _roundtrip_ok(name, ref[name], f32, bad)
    _roundtrip_ok("y", y, f32, bad)
    glayers, ghw, ghb = lay.views(ref["grads"])
    for l, (gW, gb) in enumerate(glayers):
        _roundtrip_ok(f"dW{l + 1}", gW, f32, bad)
        _roundtrip_ok(f"db{l + 1}", gb, f32, bad)
    _roundtrip_ok("dw_head", ghw, f32, bad)
    _roundtrip_ok("db_head", ghb, f32, bad)
    # accumulations; a product's quantum is (at least) the product of its factors' quanta
    H, dZ, dy = ref["H"], ref["dZ"], ref["dy"]
    for l, (W, b) in enumerate(layers):
        Wl = W[:, : H[l].shape[1]]
        _sum_ok(f"Z{l + 1}", H[l].abs() @ Wl.abs().t() + b.abs(), min(quantum(H[l]) * quantum(Wl), quantum(b)), bad)
        _sum_ok(f"dW{l + 1}", dZ[l].abs().t() @ H[l].abs(), quantum(dZ[l]) * quantum(H[l]), bad)
        _sum_ok(f"db{l + 1}", dZ[l].abs().sum(0), quantum(dZ[l]), bad)
        if l > 0:
            _sum_ok(f"dH{l}", dZ[l].abs() @ W.abs(), quantum(dZ[l]) * quantum(W), bad)
    _sum_ok("pred", H[-1].abs() @ hw.abs() + hb.abs(), min(quantum(H[-1]) * quantum(hw), quantum(hb)), bad)
    _sum_ok("dw_head", H[-1].abs().t() @ dy.abs(), quantum(H[-1]) * quantum(dy), bad)
    _sum_ok("db_head", dy.abs().sum().reshape(1), quantum(dy), bad)
    _sum_ok("loss_sum", ref["per"].abs().sum().reshape(1), quantum(ref["per"]), bad)
    # a kernel may form d = pred - y, d * d and dy_scale * d in fp32: all on the lattice
    _roundtrip_ok("pred - y", ref["pred"] - y, f32, bad)
    return bad
