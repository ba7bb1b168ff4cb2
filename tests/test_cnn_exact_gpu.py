"""Every NativeCNN path against a float64 step, BIT FOR BIT, element by element.

The data (wellflow/train/cnn_exact.py) is chosen so that bf16 / fp32 arithmetic never rounds: a
kernel, wherever it places its roundings and in whatever order it sums, must reproduce the
float64 reference cast to fp32 exactly. Every comparison is a ``torch.equal`` of a whole block
(``block_mismatches``); a failure names the block and the first differing index. The exactness
conditions are asserted on each problem before its first launch (and for all of them, without a
GPU, by tests/test_cnn_exact_cpu.py, which imports the problem list below), so a mismatch here
can only be the kernel.

Covered, each element-wise: cnn_fwd_kernel (training with and without dropout, evaluation),
cnn_bwd_kernel (both), cnn_reduce_kernel, cnn_pack_kernel, cnn_sgd_pack_kernel (csrc/cnn_fused.hip),
cnn_small_kernel (csrc/cnn_small.hip), im2col1d_kernel, loss_kernel and the gemm_kernel epilogues
with dropout and with the mask, split-K atomics included (the ``fused=False`` path).

No path needed an emulated operation: all of them match the plain float64 reference. The GEMM
path applies ``keep_scale`` to the stored activation and to dZc where the fused kernels apply it
to the dense output and to dOut; on this data both are the same numbers (the proof checks the
stored ``act * keep_scale`` and dZc as bf16 values).
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"

LOSSES = ("mse", "mae_clip")
REF = (48, 1, 100, 13, 12)          # CnnLayout(input_len, in_ch, filters, kernel, outputs): the reference's
SEED, STEP0 = 3, 5                   # engine seed; the device step counter every launch starts from

STEP_B = (1, 15, 16, 17, 128, 129, 1000, 1793)  # 1793: the empty backward chunk at 256 CUs
EDGE_F, EDGE_O, EDGE_WK, EDGE_B = (97, 100, 112), (1, 12, 16), ((48, 13), (44, 9)), (17, 129)
EDGE_LAYS = tuple((L, 1, F, k, O) for (L, k) in EDGE_WK for F in EDGE_F for O in EDGE_O)
STATE_B = (1000, 40)
EVAL_B = (1, 15, 16, 17, 129, 1000)
GEMM_LAYS = (REF, (24, 3, 20, 5, 1), (24, 3, 100, 5, 12))  # the last two: refused by the fused kernels
GEMM_B = (1, 37, 256, 600)           # dWd split 1, 1, 1, 2; dWc split 1 .. 5
SMALL_B = (4, 20, 64)
SGD = {"lr": 2.0 ** -3, "momentum": 0.5, "nesterov": True}   # the small kernel's update (zero decay)
IMAGE_O = (1, 12, 16)
# Seeds follow from (layout, B, loss); the offsets listed here replace draws of one-output
# problems in which the 16 or 17 residuals' dense-bias gradients cancelled to exactly 0
# (tests/test_cnn_exact_cpu.py requires every gradient block of every problem to be nonzero).
RESEED = {((48, 1, 112, 13, 1), 17, "mae_clip"): 1, ((44, 1, 100, 9, 1), 17, "mae_clip"): 1,
          ((48, 1, 100, 13, 1), 16, "mse"): 1}


def _r16(n):
    return (n + 15) // 16 * 16


class Problem:
    """One batch with its float64 reference. ``path``: "fused", "gemm" or "small" (which dropout
    stream draws the mask, and which roundings the proof covers)."""

    def __init__(self, lay_t, B, loss, dropout, path):
        from wellflow.models.cnn import CnnLayout, cnn_dropout_mask
        from wellflow.train import cnn_exact as cx

        self.lay_t, self.B, self.loss, self.p, self.path = lay_t, B, loss, dropout, path
        self.lay = lay = CnnLayout(*lay_t)
        seed = 1000 * lay.filters + 10 * lay.outputs + lay.input_len + 7 * B + (3 if loss == "mse" else 0)
        seed += RESEED.get((lay_t, B, loss), 0)
        self.case = case = cx.exact_cnn_case(lay, B, seed, loss, dropout)
        self.mask = None
        if dropout > 0:
            if path == "gemm":
                self.mask = cx.gemm_dropout_mask(cx.seed32(SEED), STEP0, B * lay.lout, lay.Fp, dropout)
                self.mask = self.mask.reshape(B, lay.lout, lay.Fp)
            else:
                self.mask = cnn_dropout_mask(cx.seed32(SEED), STEP0, B, lay.lout, lay.Fp)
        self.y = cx.exact_cnn_targets(case, self.mask)
        full = self.full_ref()
        self.ref = {k: full[k] for k in ("pred", "per", "loss_sum", "dout", "grads")}
        self.pred_eval = cx.cnn_forward_fp64(case.flat, case.x, lay)
        self._violations = None

    def full_ref(self):
        from wellflow.train import cnn_exact as cx

        c = self.case
        return cx.cnn_step_fp64(c.flat, c.x, self.y, c.grad_scale, self.loss, cx.CLIP, self.mask, c.keep_scale, self.lay)

    def violations(self):
        from wellflow.train.cnn_exact import CLIP, cnn_exactness_violations

        if self._violations is None:
            self._violations = cnn_exactness_violations(self.case, self.y, self.mask, self.path, CLIP,
                                                        SGD if self.path == "small" else None)
        return self._violations

    @property
    def tag(self):
        return f"layout={self.lay_t} B={self.B} {self.loss} p={self.p} {self.path}"


@functools.lru_cache(maxsize=None)
def problem(lay_t, B, loss, dropout, path) -> Problem:
    return Problem(lay_t, B, loss, dropout, path)


def all_problem_keys():
    """Every (layout, B, loss, dropout, path) this file launches (the CPU file proves each exact).
    The empty-chunk batch is listed for 256 CUs; on another device the test proves its own."""
    keys = []
    for loss in LOSSES:
        keys += [(REF, B, loss, p, "fused") for p in (0.0, 0.5) for B in STEP_B]
        keys += [(lay, B, loss, 0.5, "fused") for lay in EDGE_LAYS for B in EDGE_B]
        keys += [(REF, B, loss, 0.5, "fused") for B in STATE_B]
        keys += [(lay, B, loss, p, "gemm") for lay in GEMM_LAYS for p in (0.0, 0.5) for B in GEMM_B]
        keys += [(REF, B, loss, p, "small") for p in (0.0, 0.5) for B in SMALL_B]
    keys += [(lay, B, "mse", 0.0, "fused") for lay in EDGE_LAYS for B in EDGE_B]        # evaluation forward
    keys += [(REF, B, "mse", 0.0, "fused") for B in EVAL_B]
    keys += [((48, 1, 100, 13, O), 16, "mse", 0.0, "fused") for O in IMAGE_O]           # operand images
    return list(dict.fromkeys(keys))


# ------------------------------------------------------------------ engines and comparison
_ENGINES = {}


def engine(lay_t, loss, dropout, cap, fused=None, cached=True):
    from wellflow.models.cnn import CnnLayout, NativeCNN
    from wellflow.train.cnn_exact import CLIP, seed32

    key = (lay_t, loss, dropout, cap, fused)
    if cached and key in _ENGINES:
        return _ENGINES[key]
    eng = NativeCNN(CnnLayout(*lay_t), cap, DEV, dropout=dropout, loss=loss, clip=CLIP, seed=SEED, fused=fused)
    assert eng.seed32 == seed32(SEED)
    if cached:
        _ENGINES[key] = eng
    return eng


def load(eng, prob, poison=True) -> None:
    bad = prob.violations()
    assert not bad, f"{prob.tag}: the problem is not exact, nothing launched: {bad}"
    eng.params.copy_(prob.case.flat.float().to(DEV))
    eng.sync_weights()
    eng.rng.fill_(STEP0)
    if poison and eng.fused:  # whatever a step reads of these it must have written itself
        for buf in (eng.dout, eng.part_wd, eng.part_wc, eng.part_f):
            buf.fill_(float("nan"))


def device_xy(prob):
    x = prob.case.x.float().to(DEV)
    if prob.lay.in_ch == 1:
        x = x.reshape(prob.B, prob.lay.input_len)
    return x, prob.y.float().to(DEV)


def check(got, want, tag) -> None:
    from wellflow.train.cnn_exact import block_mismatches

    bad = block_mismatches(got, want)
    assert not bad, f"{tag}:\n  " + "\n  ".join(bad)


def fused_got(eng, prob, ls):
    torch.cuda.synchronize()
    rows = _r16(prob.B)
    gWc, gWd, gbd = prob.lay.views(eng.grads.cpu())
    return {"dout": eng.dout[: rows * 16].view(rows, 16).cpu(), "loss": ls.detach().reshape(1).cpu(), "gWc": gWc,
            "gWd": gWd, "gbd": gbd, "rng": eng.rng.cpu()}


def fused_want(prob, mult=1.0, loss_want=None):
    from wellflow.train.cnn_exact import step_blocks

    want = step_blocks(prob.ref, prob.lay, mult)
    dout = torch.zeros(_r16(prob.B), 16)  # rows >= B of the last group and columns >= outputs: exactly 0
    dout[: prob.B] = want["dout"]
    want["dout"] = dout
    if loss_want is not None:
        want["loss"] = loss_want.reshape(1).float()
    want["rng"] = torch.tensor([STEP0 + 1], dtype=torch.int64)
    return want


def fused_step(eng, prob, tag):
    load(eng, prob)
    x, y = device_xy(prob)
    ls = eng.forward_backward(x, y, prob.case.grad_scale)
    check(fused_got(eng, prob, ls), fused_want(prob), f"{prob.tag} {tag}")


# ------------------------------------------------------------------------------ fused step
@pytest.mark.parametrize("B", STEP_B)
@pytest.mark.parametrize("dropout", (0.0, 0.5))
@pytest.mark.parametrize("loss", LOSSES)
def test_cnn_fused_step(loss, dropout, B):
    """forward_backward = cnn_fwd_kernel<train> + cnn_bwd_kernel + cnn_reduce_kernel: dOut as
    [r16(B)][16] (padding rows and columns exactly zero), the loss sum, gWc with its bias column
    and all padding, gWd, gbd, and the step counter advanced by exactly one; with the engine's
    capacity larger than B and equal to B."""
    prob = problem(REF, B, loss, dropout, "fused")
    assert prob.lay.outputs == 12
    eng = engine(REF, loss, dropout, 2048)
    assert eng.fused
    fused_step(eng, prob, "capacity 2048")
    fused_step(engine(REF, loss, dropout, B, cached=False), prob, "capacity = B")


def _empty_chunk_batch():
    """(B, chunks) of the smallest batch whose last backward chunk owns no 16-window group, from
    the device's CU count (csrc/cnn_fused.hip cnn_bwd_chunks: min(CUs / 18, ceil(groups / 8))
    chunks of ceil(groups / chunks) groups)."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    nmax = max(1, cus // 18)
    for ng in range(1, 8 * nmax + 2 * nmax * nmax):
        nch = max(1, min(nmax, (ng + 7) // 8))
        gpc = (ng + nch - 1) // nch
        if (nch - 1) * gpc >= ng:
            return 16 * (ng - 1) + 1, nch
    return None, nmax


@pytest.mark.parametrize("loss", LOSSES)
def test_cnn_fused_step_empty_backward_chunk(loss):
    """The batch that leaves the last backward chunk without any group (1793 at 256 CUs: 113
    groups in 14 chunks of 9), computed from this device's CU count: the chunk writes zero
    partials, the reduce sums them."""
    from wellflow.ops.native import lib

    B, nch = _empty_chunk_batch()
    if B is None:
        pytest.skip("fewer than 36 CUs: one backward chunk, none can be empty")
    prob = problem(REF, B, loss, 0.5, "fused")
    eng = engine(REF, loss, 0.5, 2048) if B <= 2048 else engine(REF, loss, 0.5, B, cached=False)
    wd, _, _ = lib().cnn_part_sizes(B, prob.lay.fused_dims)
    assert wd == nch * 36 * 7 * 64 * 4, (wd, nch)  # the launcher uses the chunk count computed here
    ngroups = (B + 15) // 16
    assert (nch - 1) * ((ngroups + nch - 1) // nch) >= ngroups
    fused_step(eng, prob, f"{nch} chunks, the last one empty")


@pytest.mark.parametrize("B", EDGE_B)
@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("lay_t", EDGE_LAYS, ids=lambda l: f"L{l[0]}k{l[3]}-F{l[2]}-O{l[4]}")
def test_cnn_fused_layout_edges(lay_t, loss, B):
    """Every corner cnn_fused_supported admits: 97 / 100 / 112 filters x 1 / 12 / 16 outputs x
    the 48-sample window with kernel 13 and the 44-sample window with kernel 9 (other lanes hit
    the address clamps and the bounds selects), dropout 0.5."""
    prob = problem(lay_t, B, loss, 0.5, "fused")
    eng = engine(lay_t, loss, 0.5, EDGE_B[-1])
    assert eng.fused
    fused_step(eng, prob, "layout edge")


# -------------------------------------------------------------- state carried between calls
@pytest.mark.parametrize("loss", LOSSES)
def test_cnn_fused_small_batch_after_large(loss):
    """B = 1000, then B = 40 on the same engine: the stale rows of dOut and the stale partials of
    the larger step must not reach the smaller one."""
    eng = engine(REF, loss, 0.5, 1000, cached=False)
    for B in STATE_B:
        prob = problem(REF, B, loss, 0.5, "fused")
        load(eng, prob, poison=(B == STATE_B[0]))
        x, y = device_xy(prob)
        ls = eng.forward_backward(x, y, prob.case.grad_scale)
        check(fused_got(eng, prob, ls), fused_want(prob), f"{prob.tag} after {STATE_B[0]}")


@pytest.mark.parametrize("loss", LOSSES)
def test_cnn_fused_accumulates_grads_and_loss(loss):
    """zero_grads=False twice (the step counter put back, so the same mask) gives exactly twice
    the gradients; loss_into= accumulates onto what it held."""
    prob = problem(REF, 129, loss, 0.5, "fused")
    eng = engine(REF, loss, 0.5, 2048)
    load(eng, prob)
    x, y = device_xy(prob)
    acc = torch.full((1,), 3.0, device=DEV)
    eng.forward_backward(x, y, prob.case.grad_scale, zero_grads=True, loss_into=acc)
    eng.rng.fill_(STEP0)
    ls = eng.forward_backward(x, y, prob.case.grad_scale, zero_grads=False, loss_into=acc)
    assert ls is acc
    want_loss = 3.0 + 2.0 * prob.ref["loss_sum"]
    assert float(want_loss.float()) == float(want_loss)  # still an fp32 number
    check(fused_got(eng, prob, ls), fused_want(prob, 2.0, want_loss), f"{prob.tag} two accumulated steps")


@pytest.mark.parametrize("path", ("fused", "gemm"))
def test_cnn_another_step_counter_is_rejected(path):
    """Negative control on the device: the same launch from step counter STEP0 + 1 draws another
    mask, and the comparator reports the blocks the mask reaches (so the comparisons above do
    look at what the kernels wrote)."""
    from wellflow.train.cnn_exact import block_mismatches

    prob = problem(REF, 37 if path == "gemm" else 129, "mse", 0.5, path)
    eng = engine(REF, "mse", 0.5, GEMM_B[-1], fused=False) if path == "gemm" else engine(REF, "mse", 0.5, 2048)
    load(eng, prob)
    eng.rng.fill_(STEP0 + 1)
    x, y = device_xy(prob)
    ls = eng.forward_backward(x, y, prob.case.grad_scale)
    torch.cuda.synchronize()
    gWc, gWd, gbd = prob.lay.views(eng.grads.cpu())
    got = {"loss": ls.detach().reshape(1).cpu(), "gWc": gWc, "gWd": gWd, "gbd": gbd}
    want = fused_want(prob)
    bad = block_mismatches(got, {k: want[k] for k in got})
    assert sorted(line.split(":")[0] for line in bad) == ["gWc", "gWd", "gbd", "loss"], bad


# ---------------------------------------------------------------------------- eval forward
def _eval_check(lay_t, B, train_dropout):
    prob = problem(lay_t, B, "mse", 0.0, "fused")
    eng = engine(lay_t, "mse", train_dropout, max(EDGE_B[-1], 2048 if lay_t == REF else 0))
    assert eng.fused
    load(eng, prob)
    eng.pred.fill_(float("nan"))
    x, _ = device_xy(prob)
    out = eng.forward(x)
    torch.cuda.synchronize()
    got = {"pred": eng.pred[: B * 16].view(B, 16).cpu(), "rng": eng.rng.cpu(),
           "out": out.reshape(B, prob.lay.outputs).cpu()}
    want = {"pred": prob.pred_eval.float(), "rng": torch.tensor([STEP0], dtype=torch.int64),
            "out": prob.pred_eval[:, : prob.lay.outputs].float()}
    check(got, want, f"{prob.tag} eval on a dropout-{train_dropout} engine")


@pytest.mark.parametrize("B", EVAL_B)
@pytest.mark.parametrize("train_dropout", (0.0, 0.5))
def test_cnn_eval_forward(train_dropout, B):
    """forward (cnn_fwd_kernel<eval>): predictions bit for bit, padding columns zero; no mask and
    no keep scale whatever dropout the engine trains with; the step counter untouched."""
    _eval_check(REF, B, train_dropout)


@pytest.mark.parametrize("B", EDGE_B)
@pytest.mark.parametrize("lay_t", EDGE_LAYS, ids=lambda l: f"L{l[0]}k{l[3]}-F{l[2]}-O{l[4]}")
def test_cnn_eval_forward_layout_edges(lay_t, B):
    _eval_check(lay_t, B, 0.5)


# -------------------------------------------------------------------------- operand images
def _junk_padded(prob):
    """The problem's parameters with NONZERO padding: filters >= filters of both blocks and the
    dense rows j >= outputs (which both image writers must zero, not copy)."""
    lay = prob.lay
    flat = prob.case.flat.clone()
    Wc, Wd, bd = lay.views(flat)
    Wc[lay.filters:] = 0.5
    Wd.view(16, lay.lout, lay.Fp)[:, :, lay.filters:] = -0.5
    Wd[lay.outputs:] = 1.0
    return flat


def _images_got(eng):
    return {"WcA": eng.WcA.float().cpu(), "WdF": eng.WdF.float().cpu(), "WdB": eng.WdB.float().cpu()}


def _images_want(flat, lay):
    from wellflow.train.cnn_exact import cnn_images

    return {k: v.float() for k, v in cnn_images(flat, lay).items()}


@pytest.mark.parametrize("O", IMAGE_O)
def test_cnn_pack_matches_host_decoders(O):
    """cnn_pack_kernel against the host encoders of the documented layout; the dense rows
    j >= outputs hold nonzero junk in the parameters and must be zero in WdF and WdB."""
    prob = problem((48, 1, 100, 13, O), 16, "mse", 0.0, "fused")
    assert not prob.violations()
    eng = engine(prob.lay_t, "mse", 0.0, 16, cached=False)
    flat = _junk_padded(prob)
    for buf in (eng.WcA, eng.WdF, eng.WdB):
        buf.fill_(float("nan"))
    eng.params.copy_(flat.float().to(DEV))
    eng.sync_weights()
    torch.cuda.synchronize()
    check(_images_got(eng), _images_want(flat, prob.lay), f"cnn_pack outputs={O}")


@pytest.mark.parametrize("zero_grads", (True, False))
@pytest.mark.parametrize("nesterov", (True, False))
@pytest.mark.parametrize("O", IMAGE_O)
def test_cnn_sgd_pack_matches_fp64_keras_step(O, nesterov, zero_grads):
    """cnn_sgd_pack_kernel (lr 1/4, momentum 1/2, zero decay, grad_scale 1/2, lattice gradients
    and velocities: the new parameters are multiples of 1/8 below 4, bf16 numbers) against a
    float64 Keras step: parameters, velocities, the step counter, the ticket left at zero, the
    three images = the host encoders of the NEW parameters, the bucket cleared or kept."""
    from wellflow.optim.flat import FlatSGD
    from wellflow.train.cnn_exact import keras_sgd_fp64
    from wellflow.train.exact import _pick

    prob = problem((48, 1, 100, 13, O), 16, "mse", 0.0, "fused")
    assert not prob.violations()
    lay = prob.lay
    eng = engine(prob.lay_t, "mse", 0.0, 16, cached=False)
    flat = _junk_padded(prob)
    g = torch.Generator().manual_seed(O)
    grads = _pick((-4.0, -2.0, 0.0, 2.0, 4.0), (lay.numel,), g)
    vel = _pick((-0.5, 0.0, 0.5), (lay.numel,), g)
    lr, mu, gs = 0.25, 0.5, 0.5
    pn, vn = keras_sgd_fp64(flat, grads * gs, vel, lr, mu, nesterov)
    assert torch.equal(pn.to(torch.bfloat16).double(), pn) and float(pn.abs().max()) < 4.0
    opt = FlatSGD(eng.params, eng.grads, lr=lr, momentum=mu, decay=0.0, nesterov=nesterov, zero_grads=zero_grads,
                  writeback=eng)
    eng.params.copy_(flat.float().to(DEV))
    eng.grads.copy_(grads.float().to(DEV))
    opt.vel.copy_(vel.float().to(DEV))
    for buf in (eng.WcA, eng.WdF, eng.WdB):
        buf.fill_(float("nan"))
    opt.step(gs)
    torch.cuda.synchronize()
    got = _images_got(eng)
    got.update(params=eng.params.cpu(), vel=opt.vel.cpu(), grads=eng.grads.cpu(), step=opt.step_dev[:1].cpu(),
               ticket=opt.step_dev[1:2].cpu().view(torch.int32))
    want = _images_want(pn, lay)
    want.update(params=pn.float(), vel=vn.float(), grads=torch.zeros(lay.numel) if zero_grads else grads.float(),
                step=torch.ones(1), ticket=torch.zeros(1, dtype=torch.int32))
    check(got, want, f"cnn_sgd_pack outputs={O} nesterov={nesterov} zero_grads={zero_grads}")


# ------------------------------------------------------------------------------- GEMM path
@pytest.mark.parametrize("B", GEMM_B)
@pytest.mark.parametrize("dropout", (0.0, 0.5))
@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("lay_t", GEMM_LAYS, ids=lambda l: f"L{l[0]}x{l[1]}-F{l[2]}-k{l[3]}-O{l[4]}")
def test_cnn_gemm_path_step(lay_t, loss, dropout, B):
    """fused=False: im2col1d_kernel (Xcol: bias column 1, padding 0), the conv GEMM's ReLU +
    dropout epilogue (Hc = act * keep_scale, the mask from gemm_dropout_mask at the preset step
    counter), the dense GEMM (pred), loss_kernel (loss sum, dpred, gbd), the split-K atomic dWd
    and dWc GEMMs and the mask epilogue (dZc) — every gradient block with its padding."""
    prob = problem(lay_t, B, loss, dropout, "gemm")
    lay = prob.lay
    eng = engine(lay_t, loss, dropout, GEMM_B[-1], fused=False if lay_t == REF else None)
    assert not eng.fused
    load(eng, prob)
    for buf in (eng.Xcol, eng.Hc, eng.dZc, eng.pred):
        buf.fill_(float("nan"))
    x, y = device_xy(prob)
    ls = eng.forward_backward(x, y, prob.case.grad_scale)
    torch.cuda.synchronize()
    T, Kc, Fp, Op = lay.lout, lay.Kc, lay.Fp, lay.Op
    full = prob.full_ref()
    cols = torch.zeros(B, T, Kc, dtype=torch.float64)
    cols[:, :, : lay.taps] = prob.case.x.unfold(1, lay.kernel, 1).permute(0, 1, 3, 2).reshape(B, T, lay.taps)
    cols[:, :, lay.taps] = 1.0
    gWc, gWd, gbd = lay.views(eng.grads.cpu())
    rWc, rWd, rbd = lay.views(prob.ref["grads"].float())
    got = {"Xcol": eng.Xcol[: B * T * Kc].float().view(B, T, Kc).cpu(),
           "Hc": eng.Hc[: B * T * Fp].float().view(B, T, Fp).cpu(),
           "pred": eng.pred[: B * Op].view(B, Op).cpu(), "loss": ls.detach().reshape(1).cpu(),
           "dZc": eng.dZc[: B * T * Fp].float().view(B, T, Fp).cpu(),
           "gWc": gWc, "gWd": gWd, "gbd": gbd, "rng": eng.rng.cpu()}
    want = {"Xcol": cols.float(), "Hc": (full["act"] * prob.case.keep_scale).float(), "pred": prob.ref["pred"].float(),
            "loss": prob.ref["loss_sum"].reshape(1).float(), "dZc": full["dP"].float(),
            "gWc": rWc, "gWd": rWd, "gbd": rbd, "rng": torch.tensor([STEP0 + 1], dtype=torch.int64)}
    check(got, want, prob.tag)


# ---------------------------------------------------------------------- small-batch kernel
@pytest.mark.parametrize("B", SMALL_B)
@pytest.mark.parametrize("dropout", (0.0, 0.5))
@pytest.mark.parametrize("loss", LOSSES)
def test_cnn_small_kernel_one_step(loss, dropout, B):
    """fused_steps with K = 1 (cnn_small_kernel: forward, the one exchange, backward and the
    Keras SGD update in one launch) against float64 forward + backward + Keras update:
    parameters and velocities after the launch, loss_into, the step counter and rng.

    K = 2 is not added: after one update the parameters are multiples of 2^-25 or finer, the
    second step's dense outputs are sums of 1e11 and more quanta and its predictions no fp32
    numbers; the proof rejects the second step of every problem here
    (tests/test_cnn_exact_cpu.py::test_second_small_step_is_not_exact), so K > 1 stays with
    test_small_gpu.py's "K fused = K single"."""
    from wellflow.optim.flat import FlatSGD
    from wellflow.train.cnn_exact import keras_sgd_fp64

    prob = problem(REF, B, loss, dropout, "small")
    eng = engine(REF, loss, dropout, B, cached=False)
    opt = FlatSGD(eng.params, eng.grads, lr=SGD["lr"], momentum=SGD["momentum"], decay=0.0, nesterov=SGD["nesterov"],
                  zero_grads=True, writeback=eng)
    assert eng.small_steps_reason(B, opt) is None
    load(eng, prob)
    x, y = device_xy(prob)
    acc = torch.full((1,), 3.0, device=DEV)
    eng.fused_steps(x, y, B, 1, opt, prob.case.grad_scale, loss_into=acc)
    torch.cuda.synchronize()
    eng.check_device_errors()
    pn, vn = keras_sgd_fp64(prob.case.flat, prob.ref["grads"], torch.zeros(prob.lay.numel, dtype=torch.float64),
                            SGD["lr"], SGD["momentum"], SGD["nesterov"])
    want_loss = 3.0 + prob.ref["loss_sum"]
    assert float(want_loss.float()) == float(want_loss)
    pc, vc = prob.lay.views(eng.params.cpu()), prob.lay.views(opt.vel.cpu())
    pw, vw = prob.lay.views(pn.float()), prob.lay.views(vn.float())
    got = {"loss": acc.cpu(), "step": opt.step_dev[:1].cpu(), "rng": eng.rng.cpu()}
    want = {"loss": want_loss.reshape(1).float(), "step": torch.ones(1), "rng": torch.tensor([STEP0 + 1], dtype=torch.int64)}
    for i, name in enumerate(("Wc", "Wd", "bd")):
        got[f"{name} params"], want[f"{name} params"] = pc[i], pw[i]
        got[f"{name} velocities"], want[f"{name} velocities"] = vc[i], vw[i]
    check(got, want, prob.tag)
    # the operand images were refreshed from the new parameters (plain bf16 casts of them)
    assert torch.equal(eng.WcA.cpu(), pw[0].reshape(-1).to(torch.bfloat16))
