"""The float64 CNN step of wellflow/train/cnn_exact.py and the exact-arithmetic recipe, without a GPU.

* the hand-written float64 step equals torch autograd on a float64 CNN1DRegressor with the same
  explicit mask (float64 roundoff on random data; bit for bit on the lattice data, which also
  pins sign(0) = 0, the inclusive clip boundary and the ``act != 0`` mask);
* every problem tests/test_cnn_exact_gpu.py launches satisfies the exactness conditions (so the
  device must match bit for bit) and the coverage conditions (so a match means something);
* both dropout mirrors and the three operand-image encoders equal per-element loops;
* planted errors in a host replica of the fused step (organised as the kernels are: 16-window
  groups, backward chunks, the operand images) are each rejected by the comparator the GPU tests
  use.
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
