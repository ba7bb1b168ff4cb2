"""The float64 CNN step of wellflow/train/cnn_exact.py and the exact-arithmetic recipe, without a GPU.

* the hand-written float64 step equals torch autograd on a float64 CNN1DRegressor with the same
  explicit mask (float64 roundoff on random data; bit for bit on the lattice data, which also
  pins sign(0) = 0, the inclusive clip boundary and the ``act != 0`` mask);
* every problem tests/test_cnn_exact_gpu.py launches satisfies the exactness conditions (so the
  device must match bit for bit) and the coverage conditions (so a match means something);
* both dropout mirrors and the three operand-image encoders equal per-element loops;
* planted errors in a host replica of the fused step (organised as the kernels are: 16-window
  groups, backward chunks, the operand images) are each rejected by the comparator the GPU tests
  use;
* the small-batch kernel's edge layouts reach the branches they are listed for, its preset-state
  steps and its K-step launches with one live step are exact and covering, the float64 replay of
  a launch equals K calls of the one-step reference, and planted errors in that replay are each
  rejected by every launch listed for them.
"""
import importlib.util
import math
import os

import pytest
import torch

from wellflow.models.base import per_element_loss
from wellflow.models.cnn import CNN1DRegressor, CnnLayout, cnn_dropout_mask
from wellflow.train import cnn_exact as cx


def _gpu_module():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_cnn_exact_gpu.py")
    spec = importlib.util.spec_from_file_location("_cnn_exact_gpu_cases", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


GPU = _gpu_module()
KEYS = GPU.all_problem_keys()


def _key_id(k):
    return f"L{k[0][0]}x{k[0][1]}-F{k[0][2]}-k{k[0][3]}-O{k[0][4]}-B{k[1]}-{k[2]}-p{k[3]}-{k[4]}"


def _autograd(lay, flat, x, y, grad_scale, loss, clip, mask, keep_scale):
    """Float64 autograd of CNN1DRegressor with the explicit keep mask after ReLU and keep_scale
    on the dense output; gradients gathered into CnnLayout order."""
    m = CNN1DRegressor(lay.input_len, lay.in_ch, lay.filters, lay.kernel, lay.outputs, dropout=0.0).double()
    m.load_flat(flat)  # through fp32: callers pass fp32-exact parameters
    B, F, O, T = x.shape[0], lay.filters, lay.outputs, lay.lout
    h = torch.relu(m.conv(x.reshape(B, lay.input_len, lay.in_ch).transpose(1, 2))).transpose(1, 2)  # [B][T][F]
    if mask is not None:
        h = h * mask[:, :, :F].double()
    pred = keep_scale * torch.nn.functional.linear(h.reshape(B, -1), m.dense.weight) + m.dense.bias
    L = per_element_loss(loss, pred, y, clip).sum()
    (L * grad_scale).backward()
    g = torch.zeros(lay.numel, dtype=torch.float64)
    gWc, gWd, gbd = lay.views(g)
    gWc[:F, : lay.taps] = m.conv.weight.grad.permute(0, 2, 1).reshape(F, -1)
    gWc[:F, lay.taps] = m.conv.bias.grad
    gWd.view(lay.Op, T, lay.Fp)[:O, :, :F] = m.dense.weight.grad.view(O, T, F)
    gbd[:O] = m.dense.bias.grad
    return pred.detach(), L.detach(), g


@pytest.mark.parametrize("loss", ["mse", "mae_clip"])
@pytest.mark.parametrize("lay_t,B,p", [((48, 1, 100, 13, 12), 21, 0.5), ((44, 1, 97, 9, 1), 9, 0.0),
                                       ((24, 3, 20, 5, 3), 33, 0.5)])
def test_fp64_step_matches_autograd_on_random_data(lay_t, B, p, loss):
    lay = CnnLayout(*lay_t)
    flat = CNN1DRegressor(*lay_t, dropout=0.0).init_keras(seed=B).to_flat()
    with torch.no_grad():
        lay.views(flat)[2][: lay.outputs] = 0.1
        lay.views(flat)[0][: lay.filters, lay.taps] = 0.02
    flat = flat.double()  # fp32 values
    g = torch.Generator().manual_seed(B)
    x = torch.randn(B, lay.input_len, lay.in_ch, generator=g, dtype=torch.float64)
    y = 0.3 * torch.randn(B, lay.outputs, generator=g, dtype=torch.float64)
    mask = (torch.rand(B, lay.lout, lay.Fp, generator=g) >= p) if p > 0 else None
    ks = 1.0 / (1.0 - p) if p > 0 else 1.0
    clip = 0.3  # elements on both sides
    ref = cx.cnn_step_fp64(flat, x, y, 1.0 / B, loss, clip, mask, ks, lay)
    pred, L, grads = _autograd(lay, flat, x, y, 1.0 / B, loss, clip, mask, ks)
    if loss == "mae_clip":
        cut = ((pred - y).abs() > clip).double().mean().item()
        assert 0.05 < cut < 0.95
    O = lay.outputs
    # the only margin is float64 roundoff of sums in another order
    torch.testing.assert_close(ref["pred"][:, :O], pred, rtol=1e-12, atol=1e-13)
    torch.testing.assert_close(ref["loss_sum"], L, rtol=1e-12, atol=0)
    torch.testing.assert_close(ref["grads"], grads, rtol=1e-11, atol=1e-14)
    assert ref["pred"][:, O:].abs().sum() == 0 and ref["dout"][:, O:].abs().sum() == 0
    for k in ("P", "act", "dAct", "dP"):
        assert ref[k].shape == (B, lay.lout, lay.Fp)
        assert ref[k][:, :, lay.filters:].abs().sum() == 0, k


@pytest.mark.parametrize("key", KEYS, ids=_key_id)
def test_gpu_problems_are_exact_covering_and_match_autograd(key):
    """For each problem of the GPU file: the exactness conditions hold; on this data the
    hand-written step equals autograd + per_element_loss bit for bit; and the coverage conditions
    hold: a residual at 0 (from four elements on), for clipped MAE one on the boundary and one
    beyond it, a pre-activation exactly 0, every gradient block nonzero, all padding zero, and
    with dropout every (step, 16-filter block) that has at least 64 live (window, filter) units
    holds a kept-active, a dropped-active and an inactive one (the problem as a whole always)."""
    prob = GPU.problem(*key)
    assert prob.violations() == []
    c, lay = prob.case, prob.lay
    B, O, F = prob.B, lay.outputs, lay.filters
    ref = prob.full_ref()
    pred, L, grads = _autograd(lay, c.flat, c.x, prob.y, c.grad_scale, prob.loss, cx.CLIP, prob.mask, c.keep_scale)
    assert torch.equal(ref["pred"][:, :O], pred)
    assert torch.equal(ref["loss_sum"], L)
    assert torch.equal(ref["grads"], grads)
    assert torch.equal(ref["pred"][:, :O] - prob.y, c.e)  # each element has the residual it was given
    gs = c.grad_scale
    assert math.frexp(gs)[0] == 0.5 and gs <= 1.0 / 64 and gs * B * O <= 1.0  # a power of two
    # padding: filters >= F of both blocks, outputs >= O, K slots > taps
    for flat in (c.flat, ref["grads"]):
        Wc, Wd, bd = lay.views(flat)
        assert Wc[F:].abs().sum() == 0 and Wc[:, lay.taps + 1:].abs().sum() == 0
        assert Wd[O:].abs().sum() == 0 and Wd.view(lay.Op, lay.lout, lay.Fp)[:, :, F:].abs().sum() == 0
        assert bd[O:].abs().sum() == 0
    gWc, gWd, gbd = lay.views(ref["grads"])
    assert gWc[:, : lay.taps].abs().max() > 0 and gWc[:, lay.taps].abs().max() > 0
    assert gWd.abs().max() > 0 and gbd.abs().max() > 0
    e = c.e.abs()
    if B * O >= 4:
        assert (e == 0).any()
        if prob.loss == "mae_clip":
            assert (e == cx.CLIP).any() and (e > cx.CLIP).any() and ((e < cx.CLIP) & (e > 0)).any()
    P, act = ref["P"][:, :, :F], ref["act"][:, :, :F]
    assert (P == 0).any() and (P > 0).any() and (P < 0).any()
    if prob.mask is not None:
        on = P > 0
        kept, dropped = on & prob.mask[:, :, :F], on & ~prob.mask[:, :, :F]
        assert kept.any() and dropped.any()
        for b in range(lay.Fp // 16):
            live = min(F, 16 * b + 16) - 16 * b
            if B * live < 64:
                continue
            s = slice(16 * b, 16 * b + live)
            for name, m in (("kept-active", kept), ("dropped-active", dropped), ("inactive", ~on)):
                per_t = m[:, :, s].any(dim=2).any(dim=0)
                assert per_t.all(), f"block {b}: no {name} unit at steps {(~per_t).nonzero().reshape(-1).tolist()}"
        assert torch.equal(act, torch.where(kept, P, torch.zeros_like(P)))


def test_violations_are_detected():
    """The checker is not vacuous: a 9-bit input, an off-lattice target, a 9-bit dAct and an
    fp32-overflowing accumulation are each reported."""
    lay = CnnLayout()
    case = cx.exact_cnn_case(lay, 16, 1, "mse", 0.0)
    y = cx.exact_cnn_targets(case, None)
    assert cx.cnn_exactness_violations(case, y, None) == []
    bad = cx.CnnExactCase(lay, case.flat, case.x.clone(), case.e, case.grad_scale, "mse", 0.0)
    bad.x[3, 2, 0] = 1.0 + 2.0 ** -8
    assert any(v.startswith("x:") for v in cx.cnn_exactness_violations(bad, y, None))
    y2 = y.clone()
    y2[0, 0] += 2.0 ** -30
    assert cx.cnn_exactness_violations(case, y2, None) != []
    fine = cx.CnnExactCase(lay, case.flat, case.x, case.e + 2.0 ** -9, case.grad_scale, "mse", 0.0)
    assert any(v.startswith("dAct") for v in cx.cnn_exactness_violations(fine, y - 2.0 ** -9, None))
    big = cx.CnnExactCase(lay, case.flat, case.x * 2.0 ** 14 + 0.5, case.e, case.grad_scale, "mse", 0.0)
    assert cx.cnn_exactness_violations(big, y, None) != []
    # the small kernel's update: a learning rate that is no power of two leaves the lattice
    assert cx.cnn_exactness_violations(case, y, None, "small", sgd=GPU.SGD) == []
    assert cx.cnn_exactness_violations(case, y, None, "small", sgd=dict(GPU.SGD, lr=0.001)) != []


# --------------------------------------------------------------------------- dropout mirrors
def _uniform_hash_loop(seed, idx):
    M = (1 << 64) - 1
    z = (seed + idx * 0x9E3779B97F4A7C15) & M
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
    z ^= z >> 31
    return (z >> 40) / 16777216.0  # 24 bits: exact as fp32 and as a Python float


@pytest.mark.parametrize("seed,step,M,N", [(7, None, 5, 16), (cx.seed32(3), 5, 9, 32), (0x7FFFFFFF, (1 << 33) + 3, 4, 112),
                                           ((1 << 40) + 11, 1 << 62, 3, 8)])
def test_gemm_dropout_mask_equals_the_per_element_loop(seed, step, M, N):
    got = cx.gemm_dropout_mask(seed, step, M, N, 0.5)
    assert got.shape == (M, N) and got.dtype == torch.bool
    s = seed if step is None else seed ^ ((step * 0xD1B54A32D192ED03) & ((1 << 64) - 1))
    want = torch.tensor([[_uniform_hash_loop(s, m * N + n) >= 0.5 for n in range(N)] for m in range(M)])
    assert torch.equal(got, want)
    assert got.any() and not got.all()


def test_gemm_dropout_hash_wraps_at_64_bits():
    """Indices above 2^32, products that overflow 2^64 and a seed with its top bit set: the
    mask's hash (gemm_dropout_mask is vectorised over m * N + n from 0, so the large indices are
    given to the hash it calls) against Python integers."""
    import numpy as np

    idx = [0, 1, (1 << 32) - 1, (1 << 32) + 5, (1 << 40) + 123, (1 << 63) + 9, (1 << 64) - 1]
    for seed in (99, (1 << 63) + 12345, (1 << 64) - 1):
        got = cx.uniform_hash(seed, np.array(idx, dtype=np.uint64))
        assert got.dtype == np.float32
        assert [float(v) for v in got] == [_uniform_hash_loop(seed, i) for i in idx]


def _lowbias32_loop(x):
    x &= 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846CA68B) & 0xFFFFFFFF
    return x ^ (x >> 16)


@pytest.mark.parametrize("seed,step", [(cx.seed32(3), 5), (0x7FFFFFFF, (1 << 32) - 2)])
def test_cnn_dropout_mask_equals_the_per_element_loop(seed, step):
    """models/cnn.py cnn_dropout_mask at Fp = 112 against csrc/cnn_fused.hip written as a loop."""
    B, T, Fp = 3, 36, 112
    got = cnn_dropout_mask(seed, step, B, T, Fp)
    smix = _lowbias32_loop(seed ^ _lowbias32_loop(step + 0x9E3779B9))
    want = torch.zeros(B, T, Fp, dtype=torch.bool)
    for w in range(B):
        for t in range(T):
            for f in range(Fp):
                b, q, r = f >> 4, (f >> 2) & 3, f & 3
                word = _lowbias32_loop(((((w * T + t) & 0xFFFFFFFF) * 4 + q) & 0xFFFFFFFF) ^ smix)
                want[w, t, f] = bool((word >> (2 * b + (r >> 1) + 16 * (r & 1))) & 1)
    assert torch.equal(got, want)


# ---------------------------------------------------------------------------- operand images
def _images_loop(flat, lay):
    """csrc/cnn_fused.hip cnn_pack_kernel's documented layout, one element at a time."""
    Wc, Wd, _ = lay.views(flat)
    T, Fp, NFB, O = lay.lout, lay.Fp, lay.Fp // 16, lay.outputs
    WdB = torch.zeros(T, NFB, 64, 4, dtype=torch.float64)
    WdF = torch.zeros(T, NFB * 64 * 4, dtype=torch.float64)
    for t in range(T):
        for b in range(NFB):
            for lane in range(64):
                l15, q = lane & 15, lane >> 4
                for jj in range(4):
                    j = 4 * q + jj                         # WdB: lane (f = l15, q) holds Wd[4q + jj][t Fp + 16b + f]
                    WdB[t, b, lane, jj] = Wd[j, t * Fp + 16 * b + l15] if j < O else 0.0
                    v = Wd[l15, t * Fp + 16 * b + 4 * q + jj] if l15 < O else 0.0  # WdF: lane (j = l15, q)
                    if b < 6:   # pair p = b / 2: [64 lanes][8], block 2p first
                        WdF[t, 512 * (b >> 1) + 8 * lane + 4 * (b & 1) + jj] = v
                    else:       # block 6: [64 lanes][4] behind the three pairs
                        WdF[t, 1536 + 4 * lane + jj] = v
    return {"WcA": Wc.reshape(-1).clone(), "WdF": WdF.reshape(-1), "WdB": WdB.reshape(-1)}


@pytest.mark.parametrize("O", [1, 12, 16])
def test_image_encoders_equal_the_per_element_loop(O):
    lay = CnnLayout(48, 1, 100, 13, O)
    g = torch.Generator().manual_seed(O)
    flat = torch.randint(-99, 100, (lay.numel,), generator=g).double() / 8  # junk in all padding too
    got, want = cx.cnn_images(flat, lay), _images_loop(flat, lay)
    assert cx.block_mismatches(got, want) == []
    assert got["WdF"].numel() == got["WdB"].numel() == 36 * 7 * 64 * 4
    if O < 16:
        assert (lay.views(flat)[1][O:] != 0).any()


def _decode_WdF(img, lay):
    T, NFB = lay.lout, lay.Fp // 16
    v = img.reshape(T, NFB * 256)
    FB = torch.zeros(T, NFB, 64, 4, dtype=img.dtype)
    for p in range(3):
        pair = v[:, 512 * p : 512 * p + 512].reshape(T, 64, 2, 4)
        FB[:, 2 * p], FB[:, 2 * p + 1] = pair[:, :, 0], pair[:, :, 1]
    FB[:, 6] = v[:, 1536:].reshape(T, 64, 4)
    return FB.reshape(T, NFB, 4, 16, 4).permute(3, 0, 1, 2, 4).reshape(16, T * lay.Fp)


def _decode_WdB(img, lay):
    T, NFB = lay.lout, lay.Fp // 16
    return img.reshape(T, NFB, 4, 16, 4).permute(2, 4, 0, 1, 3).reshape(16, T * lay.Fp)


# --------------------------------------------------------------------------------- mutations
MUTATIONS = ("mask_shifted_by_one_filter", "pair_keep_bits_swapped", "last_partial_group_dropped",
             "keep_scale_missing_from_dout", "dwc_bias_row_omitted", "wd_fragment_pair_exchanged",
             "clip_boundary_exclusive", "backward_chunk_partial_skipped", "relu_mask_on_P_not_act")


def _replica(prob, mut=None, nch=2):
    """The fused step as the kernels organise it, in float64: the dense weights decoded from the
    WdF image (forward) and from the WdB image (backward), the batch in 16-window groups dealt
    to ``nch`` backward chunks. ``mut`` plants one error."""
    c, lay = prob.case, prob.lay
    B, O, Op, T, Fp, taps, ks = prob.B, lay.outputs, lay.Op, lay.lout, lay.Fp, lay.taps, c.keep_scale
    img = cx.cnn_images(c.flat, lay)
    WdF = img["WdF"].clone().reshape(T, -1)
    if mut == "wd_fragment_pair_exchanged":
        WdF[2, :512], WdF[2, 512:1024] = WdF[2, 512:1024].clone(), WdF[2, :512].clone()
    Wd_f, Wd_b = _decode_WdF(WdF, lay), _decode_WdB(img["WdB"], lay)
    Wc, bd = img["WcA"].reshape(Fp, lay.Kc), lay.views(c.flat)[2]
    mask = prob.mask.clone()
    if mut == "mask_shifted_by_one_filter":
        mask = mask.roll(1, dims=2)
    if mut == "pair_keep_bits_swapped":
        mask = mask.reshape(B, T, Fp // 2, 2).flip(3).reshape(B, T, Fp)
    cols = c.x.unfold(1, lay.kernel, 1).permute(0, 1, 3, 2).reshape(B, T, taps)
    P = cols @ Wc[:, :taps].t() + Wc[:, taps]
    act = torch.where(P > 0, P, torch.zeros_like(P)) * mask.double()
    h = act.reshape(B, -1)
    pred = ks * (h @ Wd_f.t()) + bd
    d = torch.zeros(B, Op, dtype=torch.float64)
    d[:, :O] = pred[:, :O] - prob.y
    if prob.loss == "mse":
        per, dout = d * d, 2.0 * c.grad_scale * d
    else:
        inside = d.abs() < cx.CLIP if mut == "clip_boundary_exclusive" else d.abs() <= cx.CLIP
        per, dout = d.abs().clamp(max=cx.CLIP), c.grad_scale * torch.sign(d) * inside.double()
    ds = dout * (1.0 if mut == "keep_scale_missing_from_dout" else ks)
    ngroups = (B + 15) // 16
    rw = torch.ones(B, dtype=torch.float64)  # which windows the backward sums
    if mut == "last_partial_group_dropped":
        rw[B // 16 * 16:] = 0.0
    rw_wd = rw.clone()
    if mut == "backward_chunk_partial_skipped":
        gpc = (ngroups + nch - 1) // nch
        rw_wd[16 * gpc * (nch - 1):] = 0.0
    dAct = (ds @ Wd_b).reshape(B, T, Fp)
    dP = dAct * ((P > 0) if mut == "relu_mask_on_P_not_act" else (act != 0)).double()
    grads = torch.zeros(lay.numel, dtype=torch.float64)
    gWc, gWd, gbd = lay.views(grads)
    gWd.copy_((ds * rw_wd[:, None]).t() @ h)
    dPw = dP * rw[:, None, None]
    gWc[:, :taps] = dPw.reshape(B * T, Fp).t() @ cols.reshape(B * T, taps)
    if mut != "dwc_bias_row_omitted":
        gWc[:, taps] = dPw.sum((0, 1))
    gbd.copy_(dout.sum(0))
    return {"dout": dout, "loss_sum": per.sum(), "grads": grads}


@pytest.mark.parametrize("loss", ["mse", "mae_clip"])
def test_replica_of_the_fused_step_matches_the_reference(loss):
    prob = GPU.problem(GPU.REF, 129, loss, 0.5, "fused")
    want = cx.step_blocks(prob.ref, prob.lay)
    assert cx.block_mismatches(cx.step_blocks(_replica(prob), prob.lay), want) == []


@pytest.mark.parametrize("mut", MUTATIONS)
def test_planted_errors_are_rejected(mut):
    """Each planted error changes at least one block the GPU tests compare, and the shared
    comparator names it."""
    prob = GPU.problem(GPU.REF, 129, "mae_clip", 0.5, "fused")
    want = cx.step_blocks(prob.ref, prob.lay)
    bad = cx.block_mismatches(cx.step_blocks(_replica(prob, mut), prob.lay), want)
    assert bad, mut
    assert all(": " in line and "first at flat index" in line for line in bad)
    if mut in ("dwc_bias_row_omitted", "last_partial_group_dropped"):
        assert any(line.startswith("gWc") for line in bad)
    if mut == "backward_chunk_partial_skipped":
        assert [line.split(":")[0] for line in bad] == ["gWd"]


def test_image_rows_not_zeroed_are_rejected():
    """The tenth planted error: an image writer that copies the dense rows j >= outputs. Only
    parameters with NONZERO padding rows show it (the GPU image tests use such parameters)."""
    lay = CnnLayout(48, 1, 100, 13, 12)
    flat = cx.exact_cnn_case(lay, 16, 5).flat.clone()
    want = cx.cnn_images(flat, lay)
    assert cx.block_mismatches(cx.cnn_images(flat, CnnLayout(48, 1, 100, 13, 16)), want) == []  # zero padding hides it
    lay.views(flat)[1][12:] = 1.0
    want = cx.cnn_images(flat, lay)
    copied = cx.cnn_images(flat, CnnLayout(48, 1, 100, 13, 16))
    bad = cx.block_mismatches(copied, want)
    assert [line.split(":")[0] for line in bad] == ["WdF", "WdB"]
    assert _decode_WdF(want["WdF"], lay)[12:].abs().sum() == 0 and _decode_WdB(want["WdB"], lay)[12:].abs().sum() == 0
    assert torch.equal(_decode_WdF(want["WdF"], lay)[:12], lay.views(flat)[1][:12])
    assert torch.equal(_decode_WdB(want["WdB"], lay)[:12], lay.views(flat)[1][:12])


@pytest.mark.parametrize("B", GPU.SMALL_B)
@pytest.mark.parametrize("loss", ["mse", "mae_clip"])
def test_second_small_step_is_not_exact(loss, B):
    """Why the small-kernel GPU test stops at K = 1: from the updated parameters the dense
    outputs are no longer sums below 2^24 quanta (fp32 conditions only; the kernel has no bf16)."""
    prob = GPU.problem(GPU.REF, B, loss, 0.0, "small")
    zero = torch.zeros(prob.lay.numel, dtype=torch.float64)
    pn, _ = cx.keras_sgd_fp64(prob.case.flat, prob.ref["grads"], zero, GPU.SGD["lr"], GPU.SGD["momentum"], GPU.SGD["nesterov"])
    c2 = cx.CnnExactCase(prob.lay, pn, prob.case.x, prob.case.e, prob.case.grad_scale, loss, 0.0)
    bad = cx.cnn_exactness_violations(c2, cx.exact_cnn_targets(c2, None), None, "small")
    assert any(v.startswith("pred:") and "quanta" in v for v in bad), bad


def test_keras_sgd_fp64_matches_flat_sgd():
    """The float64 Keras step the image and small-kernel tests use = optim/flat.py FlatSGD on the CPU."""
    from wellflow.optim.flat import FlatSGD

    g = torch.Generator().manual_seed(0)
    for nesterov in (True, False):
        p, gr, v = (torch.randn(50, generator=g, dtype=torch.float64) for _ in range(3))
        opt = FlatSGD(p.clone(), gr.clone(), lr=0.25, momentum=0.5, decay=0.0, nesterov=nesterov)
        opt.vel.copy_(v)
        opt.step(0.5)
        pn, vn = cx.keras_sgd_fp64(p, 0.5 * gr, v, 0.25, 0.5, nesterov)
        torch.testing.assert_close(opt.params, pn, rtol=1e-14, atol=1e-15)
        torch.testing.assert_close(opt.vel, vn, rtol=1e-14, atol=1e-15)


# ------------------------------------------------- the small-batch kernel: layouts, state, K steps
def test_small_kernel_layouts_reach_the_listed_branches():
    """The launcher's arithmetic (csrc/cnn_small.hip launch_cnn_small and the kernel's hop 1) for
    every (layout, B) of test_cnn_small_kernel_one_step: G = 25 / 27 / 28 workgroups, a last
    workgroup with ONE live filter at 97 / 105 / 109 filters, workers without a hop-1 output
    (nout < G) at one output and B = 4 / 20, a second trip of the hop-1 loop (nl * G > 1024) at 16
    outputs and B = 64 with both G; never more than 48 outputs per worker (red2's rows)."""
    seen = {}
    for lay_t in GPU.SMALL_LAYS:
        for B in GPU.SMALL_B:
            br = GPU.small_branches(lay_t, B)
            seen[(lay_t[2], lay_t[4], B)] = br
            assert br["G"] <= 28 and -(-br["nout"] // br["G"]) <= 48 and 4 * br["G"] <= 112
    assert {k[0]: v["G"] for k, v in seen.items()} == {97: 25, 100: 25, 105: 27, 109: 28, 112: 28}
    assert {k[0] for k, v in seen.items() if v["one_live_filter"]} == {97, 105, 109}
    assert {k for k, v in seen.items() if v["idle_workers"]} == {(97, 1, 4), (97, 1, 20), (109, 1, 4), (109, 1, 20)}
    assert {k for k, v in seen.items() if v["second_trip"]} == {(100, 16, 64), (112, 16, 64)}
    assert seen[(100, 16, 64)]["G"] * 41 == 1025 and seen[(112, 16, 64)]["G"] * 37 == 1036
    assert not seen[(100, 12, 64)]["second_trip"]  # the reference layout tops out at 768 outputs


@pytest.mark.parametrize("key", GPU.STATE_KEYS, ids=lambda k: f"F{k[0][2]}-O{k[0][4]}-B{k[1]}-{k[2]}-nesterov{k[3]}")
def test_preset_state_steps_are_exact_and_covering(key):
    """test_cnn_small_kernel_step_from_preset_state: from lattice velocities, counter 16 and decay
    2^-4 the step is exact; the velocities are live everywhere and zero on the padding; the
    carried velocity, the counter (15 and 17 give another lr_t, and no fp32-exact one) and the
    momentum rule each change the expected result."""
    lay_t, B, loss, nesterov = key
    prob = GPU.problem(lay_t, B, loss, 0.5, "small")
    lay, g, flat = prob.lay, prob.ref["grads"], prob.case.flat
    vel = GPU.state_velocities(prob)
    sgd = GPU.state_sgd(nesterov, vel)
    assert cx.cnn_exactness_violations(prob.case, prob.y, prob.mask, "small", cx.CLIP, sgd) == []
    F, O = lay.filters, lay.outputs
    Wc, Wd, bd = lay.views(vel)
    assert Wc[F:].abs().sum() == 0 and Wc[:, lay.taps + 1:].abs().sum() == 0 and bd[O:].abs().sum() == 0
    assert Wd[O:].abs().sum() == 0 and Wd.view(lay.Op, lay.lout, lay.Fp)[:, :, F:].abs().sum() == 0
    assert all(set((8 * b).reshape(-1).tolist()) >= {-4.0, 4.0, 1.0} for b in (Wc, Wd)) and bool((bd != 0).any())
    lr, mu = sgd["lr"], sgd["momentum"]
    assert cx.sgd_lr_t_fp32(lr, GPU.DECAY_STATE, GPU.IT_STATE) == lr / 2
    want = cx.keras_sgd_fp64(flat, g, vel, lr, mu, nesterov, GPU.DECAY_STATE, GPU.IT_STATE)
    for other in (cx.keras_sgd_fp64(flat, g, vel, lr, mu, nesterov, GPU.DECAY_STATE, GPU.IT_STATE - 1),
                  cx.keras_sgd_fp64(flat, g, vel, lr, mu, nesterov, GPU.DECAY_STATE, GPU.IT_STATE + 1),
                  cx.keras_sgd_fp64(flat, g, vel, lr, mu, nesterov, 0.0, GPU.IT_STATE),
                  cx.keras_sgd_fp64(flat, g, vel * 0, lr, mu, nesterov, GPU.DECAY_STATE, GPU.IT_STATE),
                  cx.keras_sgd_fp64(flat, g, vel, lr, mu, not nesterov, GPU.DECAY_STATE, GPU.IT_STATE)):
        for i, block in enumerate(lay.views(other[0].float())):   # every parameter block would show it
            assert not torch.equal(block, lay.views(want[0].float())[i])
    for it in (GPU.IT_STATE - 1, GPU.IT_STATE + 1):
        bad = cx.cnn_exactness_violations(prob.case, prob.y, prob.mask, "small", cx.CLIP, dict(sgd, iteration=it))
        assert any("lr_t" in v for v in bad)


def _sched_blocks(lay, p, v, loss_sum):
    """Parameters, velocities and the loss as the fp32 blocks the GPU test compares."""
    out = {"loss": (GPU.LOSS0 + loss_sum).reshape(1).float()}
    for i, name in enumerate(("Wc", "Wd", "bd")):
        out[f"{name} params"], out[f"{name} velocities"] = lay.views(p.float())[i], lay.views(v.float())[i]
    return out


LAUNCH_MUTATIONS = {
    # name -> which schedules (key: layout, B, loss, dropout, kinds, nesterov, preset, contiguous) MUST reject it
    "every_step_draws_the_mask_of_rng0": lambda k: k[3] > 0 and k[4].index("live") > 0,
    "lr_t_from_it0_for_every_step": lambda k: k[4].index("live") > 0,
    "step_k_reads_the_rows_of_step_k_minus_1": lambda k: k[4].index("live") > 0,
    "launch_velocities_taken_as_zero": lambda k: k[6],
    "momentum_not_applied_on_a_zero_gradient_step": lambda k: k[6] or k[4].index("live") < len(k[4]) - 1,
    "nesterov_and_plain_momentum_swapped": lambda k: True,
    "dead_step_loss_dropped": lambda k: "dead" in k[4],
}


def _launch_by_hand(s, mut=None):
    """The launch as K calls of the one-step reference and the Keras step, written out here
    (not through cnn_launch_fp64); ``mut`` plants one error."""
    c, lay = s.case, s.lay
    lr, mu, decay = s.sgd["lr"], s.sgd["momentum"], s.sgd["decay"]
    nesterov = s.sgd["nesterov"] != (mut == "nesterov_and_plain_momentum_swapped")
    p = c.flat.clone()
    v = torch.zeros_like(p) if mut == "launch_velocities_taken_as_zero" else s.vel0.clone()
    total = torch.zeros((), dtype=torch.float64)
    for k, (x, y, mask) in enumerate(s.steps):
        if mut == "every_step_draws_the_mask_of_rng0":
            mask = s.steps[0][2]
        if mut == "step_k_reads_the_rows_of_step_k_minus_1" and k > 0:
            x, y = s.steps[k - 1][0], s.steps[k - 1][1]
        ref = cx.cnn_step_fp64(p, x, y, c.grad_scale, s.loss, cx.CLIP, mask, c.keep_scale, lay)
        g = ref["grads"]
        it = s.it0 if mut == "lr_t_from_it0_for_every_step" else s.it0 + k
        if mut == "momentum_not_applied_on_a_zero_gradient_step" and not bool((g != 0).any()):
            p = p + (mu * v if nesterov else v)
        else:
            p, v = cx.keras_sgd_fp64(p, g, v, lr, mu, nesterov, decay, it)
        if not (mut == "dead_step_loss_dropped" and s.kinds[k] == "dead"):
            total = total + ref["loss_sum"]
    return _sched_blocks(lay, p, v, total)


@pytest.mark.parametrize("key", GPU.SCHEDULES, ids=GPU._sched_id)
def test_one_live_step_schedules_are_exact_and_covering(key):
    """Every launch of test_cnn_small_kernel_one_live_step: proved exact (every intermediate
    parameter and velocity of every step an fp32 number, the live step's gradient blocks all
    nonzero, each dead step's loss B * outputs * CLIP, each still step all zeros); the replay
    equals K calls of the one-step reference; and the launch holds what it is listed for."""
    s = GPU.schedule(key)
    assert s.violations() == []
    lay, B, K, kl = s.lay, s.B, s.K, s.k_live
    run = s.run
    want = _sched_blocks(lay, run["params"], run["velocities"], run["loss_sum"])
    assert cx.block_mismatches(_launch_by_hand(s), want) == []
    gpu_want = GPU.small_want(lay, run["params"], run["velocities"], run["loss_sum"], s.it0 + K, K)
    assert all(torch.equal(gpu_want[k], want[k]) for k in want)
    assert float(run["loss_sum"]) == float(run["trace"][kl]["loss"]) + s.kinds.count("dead") * B * lay.outputs * cx.CLIP
    # lr_t is lr / 2 at the live step's counter and at no other step of the launch
    lr, decay = s.sgd["lr"], s.sgd["decay"]
    assert s.it0 + kl == GPU.IT_STATE
    assert [cx.sgd_lr_t_fp32(lr, decay, s.it0 + k) == lr / 2 for k in range(K)] == [k == kl for k in range(K)]
    # distinct batches, and a table whose other rows hold other data
    for a in range(K):
        for b in range(a + 1, K):
            assert not torch.equal(s.steps[a][0], s.steps[b][0]) and not torch.equal(s.steps[a][1], s.steps[b][1])
    X, Y, rows = s.table()
    if s.contiguous:
        assert rows is None and X.shape[0] == K * B
    else:
        assert X.shape[0] == (K + 2) * B and rows.unique().numel() == K * B and not torch.equal(rows, rows.sort().values)
        for k in range(K):
            assert torch.equal(X[rows[k * B : (k + 1) * B]], s.steps[k][0].reshape(B, -1))
            assert torch.equal(Y[rows[k * B : (k + 1) * B]], s.steps[k][1])
    if s.p > 0:   # each step has a mask of its own
        assert all(not torch.equal(s.steps[a][2], s.steps[a + 1][2]) for a in range(K - 1))
    # after the live step the velocity decays by the momentum once per step and the parameters move
    mu = s.sgd["momentum"]
    tr = run["trace"]
    for k in range(kl + 1, K):
        assert torch.equal(tr[k]["velocities"] * mu, tr[k + 1]["velocities"] if k + 1 < K else run["velocities"])
        assert not torch.equal(tr[k]["params"], tr[k + 1]["params"] if k + 1 < K else run["params"])
    if not bool((s.vel0 != 0).any()):   # from zero velocities nothing moves before the live step
        assert all(torch.equal(tr[k]["params"], s.case.flat) for k in range(kl + 1))


@pytest.mark.parametrize("mut", sorted(LAUNCH_MUTATIONS))
def test_planted_launch_errors_are_rejected(mut):
    """Each planted error in the by-hand replay is rejected, by the comparator the GPU test uses
    and against the expectation it uses, by every schedule listed for it (at least one)."""
    must = [k for k in GPU.SCHEDULES if LAUNCH_MUTATIONS[mut](k)]
    assert must, mut
    for key in must:
        s = GPU.schedule(key)
        want = _sched_blocks(s.lay, s.run["params"], s.run["velocities"], s.run["loss_sum"])
        bad = cx.block_mismatches(_launch_by_hand(s, mut), want)
        assert bad, f"{mut} passes {s.tag}"
        if mut == "dead_step_loss_dropped":
            assert [line.split(":")[0] for line in bad] == ["loss"]


def test_launch_proof_is_not_vacuous():
    """cnn_launch_violations reports a dead batch whose targets sit within the clip, a still
    batch under another step's mask, a second live step and a learning rate that leaves the
    lattice."""
    s = GPU.schedule((GPU.REF, 20, "mae_clip", 0.5, ("dead", "live", "dead"), True, False, False))
    args = lambda steps, kinds=s.kinds, sgd=s.sgd: (s.case, s.vel0, steps, kinds, sgd, s.it0, cx.CLIP, GPU.LOSS0)  # noqa: E731
    assert cx.cnn_launch_violations(*args(s.steps)) == []
    x, y, mask = s.steps[2]
    near = [s.steps[0], s.steps[1], (x, y + (s.run["trace"][2]["ref"]["pred"][:, :12] - y) * 0.75, mask)]
    assert any("dead" in v for v in cx.cnn_launch_violations(*args(near)))
    assert cx.cnn_launch_violations(*args(s.steps, ("dead", "live", "live"))) != []
    assert cx.cnn_launch_violations(*args(s.steps, sgd=dict(s.sgd, lr=0.001))) != []
    m = GPU.schedule((GPU.REF, 20, "mse", 0.5, ("still", "live"), True, False, False))
    swapped = [(m.steps[0][0], m.steps[0][1], m.steps[1][2]), m.steps[1]]
    bad = cx.cnn_launch_violations(m.case, m.vel0, swapped, m.kinds, m.sgd, m.it0, cx.CLIP, GPU.LOSS0)
    assert any("still" in v for v in bad)
