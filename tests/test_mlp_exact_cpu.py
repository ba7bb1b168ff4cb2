"""The float64 MLP step of wellflow/train/exact.py and the exact-arithmetic recipe, without a GPU.

* the hand-written float64 backward equals torch autograd on a float64 MLPRegressor with
  per_element_loss as the loss (float64 roundoff on random data; bit for bit on the lattice data,
  which also pins sign(0) = 0, the inclusive clip boundary and the H > 0 mask);
* every problem tests/test_mlp_exact_gpu.py launches satisfies the exactness conditions (so the
  device must match bit for bit) and the coverage conditions (so a match means something).
"""
import importlib.util
import math
import os

import pytest
import torch

from wellflow.models.base import per_element_loss
from wellflow.models.mlp import MlpLayout, MLPRegressor, init_mlp_flat
from wellflow.train import exact as ex


def _gpu_module():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_mlp_exact_gpu.py")
    spec = importlib.util.spec_from_file_location("_mlp_exact_gpu_cases", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


GPU = _gpu_module()
KEYS = GPU.all_problem_keys()
BASE_SHAPES = sorted({(F, h, B) for (F, h, B, _, v) in KEYS if v is None and B >= 37})  # full batches


def _autograd(flat, x, y, grad_scale, loss, clip, hidden):
    F = x.shape[1]
    m = MLPRegressor(F, hidden).double()
    m.load_flat(flat)  # through fp32: callers pass fp32-exact parameters
    pred = m(x)
    L = per_element_loss(loss, pred, y, clip).sum()
    (L * grad_scale).backward()
    lay = MlpLayout(F, tuple(hidden))
    g = torch.zeros(lay.numel, dtype=torch.float64)
    layers, hw, hb = lay.views(g)
    for (W, b), lin in zip(layers, m.linears()):
        W[:, : lin.in_features].copy_(lin.weight.grad)
        b.copy_(lin.bias.grad)
    hw.copy_(m.head.weight.grad.view(-1))
    hb.copy_(m.head.bias.grad)
    return pred.detach(), L.detach(), g


@pytest.mark.parametrize("loss", ["mse", "mae_clip"])
@pytest.mark.parametrize("F,hidden,B", [(5, (256, 256), 37), (13, (32, 16, 8), 50), (9, (24,), 33), (16, (64, 32), 64)])
def test_fp64_step_matches_autograd_on_random_data(F, hidden, B, loss):
    flat = init_mlp_flat(F, hidden, seed=F).double()  # fp32 values
    g = torch.Generator().manual_seed(B)
    x = torch.randn(B, F, generator=g, dtype=torch.float64)
    y = torch.randn(B, generator=g, dtype=torch.float64)
    clip = 0.8  # rows on both sides
    ref = ex.mlp_step_fp64(flat, x, y, 1.0 / B, loss, clip, hidden=hidden)
    pred, L, grads = _autograd(flat, x, y, 1.0 / B, loss, clip, hidden)
    if loss == "mae_clip":
        cut = ((pred - y).abs() > clip).double().mean().item()
        assert 0.05 < cut < 0.95
    # the only margin is float64 roundoff of sums in another order
    torch.testing.assert_close(ref["pred"], pred, rtol=1e-13, atol=1e-14)
    torch.testing.assert_close(ref["loss_sum"], L, rtol=1e-13, atol=0)
    torch.testing.assert_close(ref["grads"], grads, rtol=1e-12, atol=1e-15)
    assert len(ref["Z"]) == len(hidden) and len(ref["H"]) == len(hidden) + 1 and len(ref["dZ"]) == len(hidden)


@pytest.mark.parametrize("key", KEYS, ids=lambda k: f"F{k[0]}-{'x'.join(map(str, k[1]))}-B{k[2]}-{k[3]}-{k[4]}")
def test_gpu_problems_are_exact_and_match_autograd(key):
    """For each problem of the GPU file: the exactness conditions hold, and on this data the
    hand-written step equals autograd + per_element_loss bit for bit (conventions at 0 and at
    the clip boundary included)."""
    prob = GPU.problem(*key)
    assert prob.violations() == []
    c = prob.case
    pred, L, grads = _autograd(c.flat, c.x, prob.y, c.grad_scale, prob.loss, prob.clip, prob.hidden)
    assert torch.equal(prob.ref["pred"], pred)
    assert torch.equal(prob.ref["loss_sum"], L)
    assert torch.equal(prob.ref["grads"], grads)
    assert torch.equal(prob.ref["pred"] - prob.y, c.e)  # each row has the residual it was given
    gs = c.grad_scale
    assert math.frexp(gs)[0] == 0.5 and gs * prob.B <= 1.0  # a power of two
    # padding columns of W1 and of its gradient are exactly zero
    for flat in (c.flat, prob.ref["grads"]):
        W1 = prob.lay.views(flat)[0][0][0]
        assert W1[:, prob.F:].abs().sum().item() == 0.0
    # every gradient block is nonzero
    gl, ghw, ghb = prob.lay.views(prob.ref["grads"])
    for l, (gW, gb) in enumerate(gl):
        assert gW.abs().max().item() > 0 and gb.abs().max().item() > 0, f"layer {l + 1}"
    assert ghw.abs().max().item() > 0 and ghb.abs().max().item() > 0


@pytest.mark.parametrize("F,hidden,B", BASE_SHAPES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_gpu_problems_cover_the_edges(F, hidden, B):
    """Coverage of the full-batch problems (B >= 37): rows inside, on and beyond the clip and
    with e = 0, pre-activations exactly 0 in every layer, 20-80 % of each layer's units on."""
    prob = GPU.problem(F, hidden, B, "mae_clip")
    e = prob.case.e.abs()
    assert (e < prob.clip).any() and (e == prob.clip).any() and (e > prob.clip).any() and (e == 0).any()
    for l, z in enumerate(prob.ref["Z"]):
        on = (z > 0).double().mean().item()
        assert 0.2 <= on <= 0.8, f"layer {l + 1} on-fraction {on:.3f}"
        assert (z == 0).any(), f"layer {l + 1}: no pre-activation exactly 0"
    # the gradient is dense enough to see a wrong element: most entries of each block nonzero
    gl, ghw, _ = prob.lay.views(prob.ref["grads"])
    for l, (gW, gb) in enumerate(gl):
        gWl = gW[:, : prob.F] if l == 0 else gW
        assert (gWl != 0).double().mean().item() > 0.5 and (gb != 0).double().mean().item() > 0.5, f"layer {l + 1}"
    assert (ghw != 0).double().mean().item() > 0.5


def test_violations_are_detected():
    """The checker is not vacuous: a 9-bit input, an off-lattice target and an fp32-overflowing
    accumulation are each reported."""
    case = ex.exact_mlp_case(8, (256, 256), 64, 1)
    y = ex.exact_targets(case)
    assert ex.exactness_violations(case, y, "mse") == []
    bad = ex.ExactCase(case.lay, case.flat, case.x.clone(), case.e, case.grad_scale)
    bad.x[3, 2] = 1.0 + 2.0 ** -8
    assert any(v.startswith("x:") for v in ex.exactness_violations(bad, y, "mse"))
    y2 = y.clone()
    y2[0] += 2.0 ** -30
    assert ex.exactness_violations(case, y2, "mse") != []
    big = ex.ExactCase(case.lay, case.flat, case.x * 2.0 ** 12 + 0.5, case.e, case.grad_scale)
    assert ex.exactness_violations(big, y, "mse") != []
    assert ex.quantum(torch.tensor([0.75, 2.0, -0.5])) == 0.25 and ex.quantum(torch.zeros(3)) == 1.0
