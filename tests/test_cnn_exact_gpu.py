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
          ((48, 1, 100, 13, 1), 16, "mse"): 1, ((48, 1, 97, 13, 1), 20, "mae_clip"): 1,
          ((48, 1, 97, 13, 1), 20, "mse"): 1, ((48, 1, 109, 13, 1), 20, "mse"): 1,
          ((48, 1, 109, 13, 1), 64, "mae_clip"): 1}

# The small-batch kernel (csrc/cnn_small.hip): G = ceil(filters / 4) workgroups of 4 filters.
# 97, 105 and 109 filters leave ONE live filter in the last workgroup; G = 25 / 27 / 28.
SMALL_EDGE_LAYS = tuple((48, 1, F, 13, O) for F, O in ((97, 1), (100, 16), (105, 12), (109, 1), (112, 16)))
SMALL_LAYS = (REF,) + SMALL_EDGE_LAYS
BIG, TINY = (48, 1, 112, 13, 16), (48, 1, 97, 13, 1)   # with B = 64: hop 1's second trip; with B = 4: idle workers
LOSS0 = 3.0                          # what loss_into holds before every small-kernel launch
IT_STATE, DECAY_STATE = 16, 2.0 ** -4   # 1 + decay * it = 2: lr_t = lr / 2 exactly, and for no other counter
STATE_KEYS = tuple((lay_t, B, loss, nes) for (lay_t, B) in ((REF, 20), (BIG, 64)) for loss in LOSSES
                   for nes in (True, False))
KERAS = {"lr": 0.001, "momentum": 0.99, "decay": 1e-6}   # the reference's optimizer (off the lattice)
KERAS_IT = (0, 1, 10 ** 6)


def small_branches(lay_t, B) -> dict:
    """What the launcher and the kernel compute from (filters, outputs, B): the grid G, the
    number of dense outputs, whether workgroups wk >= nout idle through hop 1 (nl = 0) and
    whether workgroup 0's hop-1 loop over nl * G (output, share) pairs takes a second trip."""
    G = (lay_t[2] + 3) // 4
    nout = B * lay_t[4]
    nl0 = (nout + G - 1) // G
    return {"G": G, "nout": nout, "idle_workers": nout < G, "second_trip": nl0 * G > 1024,
            "one_live_filter": lay_t[2] % 4 == 1}


def _schedules():
    """(layout, B, loss, dropout, kinds, nesterov, preset velocities, contiguous rows) of every
    one-live-step launch below."""
    out = []
    d, s, l = "dead", "still", "live"
    for lay_t, B in ((REF, 20), (BIG, 64), (TINY, 4)):
        for kinds in ((l, d, d), (d, l, d), (d, d, l), (d, d, d, l)):
            out.append((lay_t, B, "mae_clip", 0.5, kinds, True, False, False))
        out.append((lay_t, B, "mse", 0.5, (s, s, l), True, False, False))
        out.append((lay_t, B, "mse", 0.5, (s, l), True, False, False))
        out.append((lay_t, B, "mae_clip", 0.5, (l, d, d), True, True, False))    # from the preset velocities
    out.append((REF, 20, "mae_clip", 0.0, (d, l, d), True, False, False))        # no dropout, once per loss
    out.append((REF, 20, "mse", 0.0, (s, l), True, False, False))
    out.append((REF, 20, "mae_clip", 0.5, (l, d, d), False, False, False))       # plain momentum
    out.append((REF, 20, "mae_clip", 0.5, (l, d, d), False, True, False))
    out.append((REF, 20, "mae_clip", 0.5, (d, l, d), True, False, True))         # rows=None
    out.append((REF, 20, "mse", 0.5, (s, s, l), True, False, True))
    return tuple(out)


SCHEDULES = _schedules()


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
        keys += [(lay, B, loss, p, "small") for lay in SMALL_LAYS for p in (0.0, 0.5) for B in SMALL_B]
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
class Schedule:
    """One K-step launch in which exactly one step is live (wellflow/train/cnn_exact.py): the live
    batch is the "small" problem of (layout, B, loss, dropout) with its targets redrawn under the
    mask of ITS step, the others are distinct dead (clipped MAE) or still (MSE) batches. decay =
    2^-4 and the counter preset to 16 - k_live, so lr_t is lr / 2 exactly at the live step only if
    the kernel uses it0 + k. The batches are scattered through ``rows`` over a table of (K + 2) B
    rows whose other rows hold other data, or laid out contiguously (``rows`` None)."""

    def __init__(self, lay_t, B, loss, dropout, kinds, nesterov, preset, contiguous):
        from wellflow.models.cnn import cnn_dropout_mask
        from wellflow.train import cnn_exact as cx

        self.key = (lay_t, B, loss, dropout, kinds, nesterov, preset, contiguous)
        self.lay_t, self.B, self.loss, self.p, self.kinds, self.contiguous = lay_t, B, loss, dropout, kinds, contiguous
        prob = problem(lay_t, B, loss, dropout, "small")
        self.case, self.lay = case, lay = prob.case, prob.lay
        self.K, self.k_live = len(kinds), kinds.index("live")
        self.it0 = IT_STATE - self.k_live
        self.sgd = {"lr": SGD["lr"], "momentum": SGD["momentum"], "nesterov": nesterov, "decay": DECAY_STATE}
        seed = 7919 * lay.filters + 13 * B + self.K
        self.vel0 = cx.lattice_velocities(lay, seed) if preset else torch.zeros(lay.numel, dtype=torch.float64)
        self.steps = []
        p, v = case.flat, self.vel0   # the state each step starts from: a dead batch's targets follow it
        for k, kind in enumerate(kinds):
            mask = cnn_dropout_mask(cx.seed32(SEED), STEP0 + k, B, lay.lout, lay.Fp) if dropout > 0 else None
            if kind == "live":
                x, y = case.x, cx.exact_cnn_targets(case, mask)
            else:
                x = cx.exact_cnn_case(lay, B, seed + 101 * (k + 1), loss, dropout).x
                y = (cx.dead_targets(p, x, mask, case.keep_scale, lay, seed + k) if kind == "dead" else
                     cx.still_targets(p, x, mask, case.keep_scale, lay))
            self.steps.append((x, y, mask))
            one = cx.cnn_launch_fp64(p, v, self.steps[-1:], case.grad_scale, loss, cx.CLIP, case.keep_scale, lay, self.sgd,
                                     self.it0 + k)
            p, v = one["params"], one["velocities"]
        self.run = cx.cnn_launch_fp64(case.flat, self.vel0, self.steps, case.grad_scale, loss, cx.CLIP, case.keep_scale,
                                      lay, self.sgd, self.it0)
        self._violations = None

    def violations(self):
        from wellflow.train.cnn_exact import CLIP, cnn_launch_violations

        if self._violations is None:
            self._violations = cnn_launch_violations(self.case, self.vel0, self.steps, self.kinds, self.sgd, self.it0,
                                                     CLIP, LOSS0)
        return self._violations

    def table(self, steps=None):
        """(X [N][48], Y [N][outputs], rows or None), float64 / int64 on the host."""
        from wellflow.train.cnn_exact import X_VALUES
        from wellflow.train.exact import _pick

        steps = self.steps if steps is None else steps
        xs = torch.cat([s[0].reshape(self.B, -1) for s in steps])
        ys = torch.cat([s[1] for s in steps])
        if self.contiguous:
            return xs, ys, None
        g = torch.Generator().manual_seed(17 * self.B + self.K)
        N = (self.K + 2) * self.B
        X, Y = _pick(X_VALUES, (N, self.lay.input_len), g), _pick(X_VALUES, (N, self.lay.outputs), g)
        rows = torch.randperm(N, generator=g)[: self.K * self.B]
        X[rows], Y[rows] = xs, ys
        return X, Y, rows

    @property
    def tag(self):
        return (f"layout={self.lay_t} B={self.B} {self.loss} p={self.p} {'-'.join(self.kinds)} "
                f"nesterov={self.sgd['nesterov']} it0={self.it0}")


@functools.lru_cache(maxsize=None)
def schedule(key) -> Schedule:
    return Schedule(*key)


def _sched_id(k):
    return (f"F{k[0][2]}-O{k[0][4]}-B{k[1]}-{k[2]}-p{k[3]}-{'-'.join(k[4])}" + ("" if k[5] else "-plain")
            + ("-preset" if k[6] else "") + ("-contiguous" if k[7] else ""))


GRADS_FILL = 7.0   # the gradient bucket before a small-kernel launch (which must not write it)


def small_engine(lay_t, B, loss, dropout, sgd):
    """A fresh engine of capacity B with a FlatSGD of ``sgd`` (lr, momentum, nesterov, decay)."""
    from wellflow.optim.flat import FlatSGD

    eng = engine(lay_t, loss, dropout, B, cached=False)
    opt = FlatSGD(eng.params, eng.grads, lr=sgd["lr"], momentum=sgd["momentum"], decay=sgd.get("decay", 0.0),
                  nesterov=sgd["nesterov"], zero_grads=True, writeback=eng)
    assert eng.small_steps_reason(B, opt) is None
    return eng, opt


def small_launch(eng, opt, flat, vel, it0, X, Y, rows, B, K, grad_scale):
    """Parameters, velocities, both counters and the dropout step preset; then ONE launch of K
    steps with loss_into starting from LOSS0. Returns the blocks to compare."""
    eng.params.copy_(flat.float().to(DEV))
    eng.sync_weights()
    eng.rng.fill_(STEP0)
    eng.grads.fill_(GRADS_FILL)
    opt.vel.copy_(vel.float().to(DEV))
    opt.step_dev.zero_()
    opt.step_dev[0] = float(it0)
    opt.iterations = it0
    acc = torch.full((1,), LOSS0, device=DEV)
    rows = None if rows is None else rows.to(DEV)
    eng.fused_steps(X.float().to(DEV), Y.float().to(DEV), B, K, opt, grad_scale, rows=rows, loss_into=acc)
    torch.cuda.synchronize()
    eng.check_device_errors()
    got = {"loss": acc.cpu(), "step": opt.step_dev[:1].cpu(), "ticket": opt.step_dev[1:].cpu(), "rng": eng.rng.cpu(),
           "iterations": torch.tensor([opt.iterations]), "grads": eng.grads.cpu(), "WcA": eng.WcA.cpu()}
    pc, vc = eng.lay.views(eng.params.cpu()), eng.lay.views(opt.vel.cpu())
    for i, name in enumerate(("Wc", "Wd", "bd")):
        got[f"{name} params"], got[f"{name} velocities"] = pc[i], vc[i]
    return got


def small_want(lay, pn, vn, loss_sum, it_end, K):
    """The float64 parameters / velocities after the launch as the fp32 blocks small_launch
    returns (all padding included: zero), the loss on top of LOSS0, both counters, the dropout
    step, the refreshed conv image (a bf16 cast of the new conv block) and what the launch must
    leave alone: the gradient bucket and the optimizer's ticket words."""
    want_loss = LOSS0 + loss_sum
    assert float(want_loss.float()) == float(want_loss)
    want = {"loss": want_loss.reshape(1).float(), "step": torch.tensor([float(it_end)]), "ticket": torch.zeros(3),
            "rng": torch.tensor([STEP0 + K], dtype=torch.int64), "iterations": torch.tensor([it_end]),
            "grads": torch.full((lay.numel,), GRADS_FILL)}
    pw, vw = lay.views(pn.float()), lay.views(vn.float())
    for i, name in enumerate(("Wc", "Wd", "bd")):
        want[f"{name} params"], want[f"{name} velocities"] = pw[i], vw[i]
    want["WcA"] = pw[0].reshape(-1).to(torch.bfloat16)
    return want


def _small_one_step(lay_t, loss, dropout, B):
    from wellflow.train.cnn_exact import keras_sgd_fp64

    br = small_branches(lay_t, B)
    assert br["G"] == {97: 25, 100: 25, 105: 27, 109: 28, 112: 28}[lay_t[2]]
    assert br["one_live_filter"] == (lay_t[2] in (97, 105, 109))
    assert br["idle_workers"] == (lay_t[4] == 1 and B <= 20)          # nout < G: workers with nl = 0
    assert br["second_trip"] == (lay_t[4] == 16 and B == 64)          # nl * G > 1024
    prob = problem(lay_t, B, loss, dropout, "small")
    bad = prob.violations()
    assert not bad, f"{prob.tag}: the problem is not exact, nothing launched: {bad}"
    eng, opt = small_engine(lay_t, B, loss, dropout, SGD)
    zero = torch.zeros(prob.lay.numel, dtype=torch.float64)
    got = small_launch(eng, opt, prob.case.flat, zero, 0, prob.case.x.reshape(B, -1), prob.y, None, B, 1,
                       prob.case.grad_scale)
    pn, vn = keras_sgd_fp64(prob.case.flat, prob.ref["grads"], zero, SGD["lr"], SGD["momentum"], SGD["nesterov"])
    check(got, small_want(prob.lay, pn, vn, prob.ref["loss_sum"], 1, 1), f"{prob.tag} {br}")


@pytest.mark.parametrize("B", SMALL_B)
@pytest.mark.parametrize("dropout", (0.0, 0.5))
@pytest.mark.parametrize("loss", LOSSES)
def test_cnn_small_kernel_one_step(loss, dropout, B):
    """fused_steps with K = 1 (cnn_small_kernel: forward, the one exchange, backward and the
    Keras SGD update in one launch) against float64 forward + backward + Keras update:
    parameters and velocities of all three blocks with their padding, loss_into from a nonzero
    start, both step counters, rng, the refreshed WcA; the gradient bucket and the ticket words
    untouched.

    Two LIVE steps cannot be exact: after one update the parameters are multiples of 2^-25 or
    finer, the second step's dense outputs are sums of 1e11 and more quanta and its predictions
    no fp32 numbers (tests/test_cnn_exact_cpu.py::test_second_small_step_is_not_exact). Steps
    k >= 1 of a launch are pinned by test_cnn_small_kernel_one_live_step below (one live step
    among batches whose gradient is exactly zero), several live steps on random data by
    test_small_gpu.py's "K fused = K single"."""
    _small_one_step(REF, loss, dropout, B)


@pytest.mark.parametrize("B", SMALL_B)
@pytest.mark.parametrize("dropout", (0.0, 0.5))
@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("lay_t", SMALL_EDGE_LAYS, ids=lambda l: f"F{l[2]}-O{l[4]}")
def test_cnn_small_kernel_one_step_edge_layouts(lay_t, loss, dropout, B):
    """The same on the edges of what small_steps_reason and the launcher admit (97 .. 112 filters
    x 1 .. 16 outputs): G = 25, 27 and 28 workgroups, ONE live filter in the last workgroup (97,
    105, 109), workgroups without a hop-1 output (nout < G: one output, B = 4 and 20) and the
    second trip of the hop-1 loop (nl * G > 1024: 16 outputs, B = 64); each case asserts the
    branch it is listed for from B, O and G as the launcher computes them."""
    _small_one_step(lay_t, loss, dropout, B)


def state_sgd(nesterov, vel):
    return {"lr": SGD["lr"], "momentum": SGD["momentum"], "nesterov": nesterov, "decay": DECAY_STATE,
            "iteration": IT_STATE, "velocities": vel}


def state_velocities(prob):
    from wellflow.train.cnn_exact import lattice_velocities

    return lattice_velocities(prob.lay, 31 * prob.lay.filters + prob.B)


@pytest.mark.parametrize("lay_t,B,loss,nesterov", STATE_KEYS, ids=lambda v: f"F{v[2]}-O{v[4]}" if isinstance(v, tuple) else str(v))
def test_cnn_small_kernel_step_from_preset_state(lay_t, B, loss, nesterov):
    """One step from a state that is not zero, bit for bit: velocities preset on the lattice
    (multiples of 1/8, zero on the padding), Nesterov and plain momentum, the device counter
    preset to 16 with decay 2^-4 (lr_t = lr / 2 exactly; any other counter gives another lr_t)."""
    from wellflow.train.cnn_exact import CLIP, cnn_exactness_violations, keras_sgd_fp64

    prob = problem(lay_t, B, loss, 0.5, "small")
    vel = state_velocities(prob)
    sgd = state_sgd(nesterov, vel)
    bad = cnn_exactness_violations(prob.case, prob.y, prob.mask, "small", CLIP, sgd)
    assert not bad, f"{prob.tag}: not exact from the preset state, nothing launched: {bad}"
    eng, opt = small_engine(lay_t, B, loss, 0.5, sgd)
    got = small_launch(eng, opt, prob.case.flat, vel, IT_STATE, prob.case.x.reshape(B, -1), prob.y, None, B, 1,
                       prob.case.grad_scale)
    pn, vn = keras_sgd_fp64(prob.case.flat, prob.ref["grads"], vel, sgd["lr"], sgd["momentum"], nesterov, DECAY_STATE,
                            IT_STATE)
    assert not torch.equal(vn, keras_sgd_fp64(prob.case.flat, prob.ref["grads"], vel * 0, sgd["lr"], sgd["momentum"],
                                              nesterov, DECAY_STATE, IT_STATE)[1])
    check(got, small_want(prob.lay, pn, vn, prob.ref["loss_sum"], IT_STATE + 1, 1), f"{prob.tag} nesterov={nesterov}")


@pytest.mark.parametrize("it", KERAS_IT)
@pytest.mark.parametrize("nesterov", (True, False))
@pytest.mark.parametrize("lay_t,B", ((REF, 20), (BIG, 64)), ids=("F100-O12-B20", "F112-O16-B64"))
def test_cnn_small_kernel_keras_decay_within_bound(lay_t, B, nesterov, it):
    """The reference's optimizer (lr 0.001, momentum 0.99, decay 1e-6) with the counter at 0, 1
    and 10^6, from lattice velocities: the gradient is exact, only the update rounds, so every
    parameter and velocity lies within train/optim_ref.py sgd_tol of sgd_fp64 (the bound derived
    for this very formula: the kernel's ``sgd`` lambda); the padding, where the bound is 0, is
    unchanged. Measured worst error / bound on an MI355X: see COVERAGE.md row K8."""
    from wellflow.train import optim_ref as R

    prob = problem(lay_t, B, "mae_clip", 0.5, "small")
    assert not prob.violations()
    vel = state_velocities(prob)
    lr, mu, decay = R.f32(KERAS["lr"]), R.f32(KERAS["momentum"]), R.f32(KERAS["decay"])
    eng, opt = small_engine(lay_t, B, "mae_clip", 0.5, dict(KERAS, nesterov=nesterov))
    got = small_launch(eng, opt, prob.case.flat, vel, it, prob.case.x.reshape(B, -1), prob.y, None, B, 1,
                       prob.case.grad_scale)
    g = prob.ref["grads"]
    pn, vn = R.sgd_fp64(prob.case.flat, g, vel, it, lr, mu, nesterov, decay)
    tol_p, tol_v = R.sgd_tol(pn, g, vel, vn, it, lr, mu, nesterov, decay)
    gp = torch.cat([got[f"{n} params"].reshape(-1) for n in ("Wc", "Wd", "bd")]).double()
    gv = torch.cat([got[f"{n} velocities"].reshape(-1) for n in ("Wc", "Wd", "bd")]).double()
    worst = {}
    for name, have, ref, tol in (("p", gp, pn, tol_p), ("vel", gv, vn, tol_v)):
        err = (have - ref).abs()
        live = tol > 0
        worst[name] = float((err[live] / tol[live]).max())
        assert bool((err[~live] == 0).all()), f"{name}: an element with a zero bound changed"
    print(f"[cnn_small sgd] F={lay_t[2]} O={lay_t[4]} B={B} nesterov={nesterov} it={it} worst error / bound: "
          f"p {worst['p']:.3f} vel {worst['vel']:.3f}")
    assert worst["p"] <= 1.0 and worst["vel"] <= 1.0, worst
    rest = small_want(prob.lay, pn, vn, prob.ref["loss_sum"], it + 1, 1)
    rest = {k: rest[k] for k in ("loss", "step", "ticket", "rng", "iterations", "grads")}
    rest["WcA"] = got["Wc params"].reshape(-1).to(torch.bfloat16)   # the image of what the kernel wrote
    check(got, rest, f"{prob.tag} keras it={it}")


@pytest.mark.parametrize("ids", ("inside", "clamped"))
@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("lay_t,B", ((REF, 20), (BIG, 64)), ids=("F100-O12-B20", "F112-O16-B64"))
def test_cnn_small_kernel_rows(lay_t, B, loss, ids):
    """The batch read through ``rows`` from a table of 3 B rows whose other rows hold other
    data, the batch's windows at scattered positions that include the first and the last row.
    "clamped": the ids of those two are -3 and N + 5; the kernel clamps every id into [0, N), so
    the launch equals the one with ids 0 and N - 1."""
    from wellflow.train.cnn_exact import X_VALUES, keras_sgd_fp64
    from wellflow.train.exact import _pick

    prob = problem(lay_t, B, loss, 0.5, "small")
    assert not prob.violations()
    N = 3 * B
    g = torch.Generator().manual_seed(23)
    X, Y = _pick(X_VALUES, (N, prob.lay.input_len), g), _pick(X_VALUES, (N, prob.lay.outputs), g)
    rows = torch.randperm(N - 2, generator=g)[:B] + 1
    rows[3], rows[B - 1] = 0, N - 1
    X[rows], Y[rows] = prob.case.x.reshape(B, -1), prob.y
    assert not torch.equal(X[:B], prob.case.x.reshape(B, -1)) and not torch.equal(rows, rows.sort().values)
    if ids == "clamped":
        rows[3], rows[B - 1] = -3, N + 5
    eng, opt = small_engine(lay_t, B, loss, 0.5, SGD)
    zero = torch.zeros(prob.lay.numel, dtype=torch.float64)
    got = small_launch(eng, opt, prob.case.flat, zero, 0, X, Y, rows, B, 1, prob.case.grad_scale)
    pn, vn = keras_sgd_fp64(prob.case.flat, prob.ref["grads"], zero, SGD["lr"], SGD["momentum"], SGD["nesterov"])
    check(got, small_want(prob.lay, pn, vn, prob.ref["loss_sum"], 1, 1), f"{prob.tag} rows {ids}")


@pytest.mark.parametrize("key", SCHEDULES, ids=_sched_id)
def test_cnn_small_kernel_one_live_step(key):
    """K = 2 .. 4 steps in ONE launch, exactly one of them live (class Schedule), against the
    float64 replay of the launch, bit for bit: this pins, for steps k >= 1, the dropout step
    rng0 + k (a still step under another mask is live; the live step's targets are drawn under its
    own), it0 + k (lr_t is lr / 2 only at the live step's counter), ``rows[k B + w]`` and the
    two-ahead prefetch (distinct batches), both parities of the exchange buffers twice (K = 4), and
    the momentum carried in LDS: after [live, dead, dead] the velocity has decayed twice and the
    parameters have moved each time. Each dead step adds exactly B * outputs * CLIP to the loss."""
    s = schedule(key)
    bad = s.violations()
    assert not bad, f"{s.tag}: the launch is not exact, nothing launched: {bad}"
    eng, opt = small_engine(s.lay_t, s.B, s.loss, s.p, s.sgd)
    X, Y, rows = s.table()
    got = small_launch(eng, opt, s.case.flat, s.vel0, s.it0, X, Y, rows, s.B, s.K, s.case.grad_scale)
    run = s.run
    check(got, small_want(s.lay, run["params"], run["velocities"], run["loss_sum"], s.it0 + s.K, s.K), s.tag)
