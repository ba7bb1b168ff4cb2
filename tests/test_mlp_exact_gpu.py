"""Every NativeMLP training and inference path against a float64 step, BIT FOR BIT.

The data (wellflow/train/exact.py) is chosen so that bf16 / fp32 arithmetic never rounds: a
kernel path, wherever it places its roundings and in whatever order it sums, must reproduce the
float64 reference cast to fp32 exactly — predictions, loss sum and each of the six gradient
blocks (the zero padding columns of dW1 included). Every comparison is a ``torch.equal``; a
failure names the block and the first differing index. The exactness conditions are asserted on
each problem before its first launch (and for all of them, without a GPU, by
tests/test_mlp_exact_cpu.py, which imports the problem list below), so a mismatch here can only
be the kernel.

No path needed an emulated operation: all of them match the plain float64 reference.
"""
import contextlib
import functools
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"

HID = (256, 256)
LOSSES = ("mse", "mae_clip")
CAP = 512  # engine capacity in rows (>= every B below)

STEP_F, STEP_B = (5, 16, 24, 32), (64, 128, 192, 256)  # B = 64, 192 end the 128-row kernel in a half pass
WIDE_F, WIDE_B = (33, 40, 64), (64, 192)
TAIL_F, TAIL_B = (5, 16, 40), (1, 37, 63, 65, 300)
OTHER_HID, OTHER_F, OTHER_B = ((256, 128), (128,)), 13, (37, 300)
PROBE_F, PROBE_B, PROBE_ROWS = 16, 192, (0, 63, 64, 127, 128, 191)
CALL_F, CALL_B = (5, 16), 192
INFER_F, INFER_B = (5, 16, 40), (1, 63, 64, 65, 300)

# Seeds are per (F, hidden, B); the two listed here replace draws in which a one-row batch drew
# a residual without a gradient (e = 0 or beyond the clip). tests/test_mlp_exact_cpu.py checks
# the coverage conditions for every problem (a clipped-MAE db3 may also cancel to exactly 0).
SEEDS = {(5, HID, 1): 506, (16, HID, 1): 1604}


def seed_for(F, hidden, B):
    return SEEDS.get((F, tuple(hidden), B), 100 * F + B + len(hidden))


# the step-path switches: attributes flipped on a default engine / environment at construction
STEP_PATHS = {
    "default": ({}, {}),
    "step64": ({"w2t": None}, {}),
    "rowmajor_dz2": ({"dw2_frag": False}, {}),
    "pair": ({"step_fused": False}, {}),
    "dw2_gemm": ({"dw2_gemm": True}, {}),
    "stored_h1": ({"recompute_h1": False}, {}),
    "gemm_bwd": ({"fused_bwd": False}, {}),
    "per_layer": ({"fused": False}, {}),
    "h2_stored": ({"mask_h2": False}, {}),
    "direct_atomics": ({}, {"WELLFLOW_MLP_SPREAD": "0"}),
    "env_step64": ({}, {"WELLFLOW_MLP_STEP128": "0"}),
}
# which of them keep the H1-free step (the one-launch step, or for MSE the kernel pair) at
# B % 64 == 0, Fp <= 32; the others must reach the multi-launch path (_recompute_ok)
H1_FREE = {"mse": {"default", "step64", "rowmajor_dz2", "pair", "dw2_gemm", "direct_atomics", "env_step64"},
           "mae_clip": {"default", "step64", "rowmajor_dz2", "env_step64"}}


class Problem:
    """One batch with its float64 reference; ``variant``: None, ("probe", row), or
    ("rows", "perm" | "repeat") = a B-row index into a 3B-row dataset."""

    def __init__(self, F, hidden, B, loss, variant=None):
        from wellflow.train import exact as ex

        self.F, self.hidden, self.B, self.loss, self.variant = F, tuple(hidden), B, loss, variant
        rows = variant is not None and variant[0] == "rows"
        case = ex.exact_mlp_case(F, hidden, 3 * B if rows else B, seed_for(F, hidden, B))
        case.grad_scale = ex.exact_grad_scale(B)
        if variant is not None and variant[0] == "probe":
            # every row but one muted: e = 4 is beyond the clip, e = 0 has no MSE gradient
            r = variant[1]
            e = torch.full_like(case.e, 4.0 if loss == "mae_clip" else 0.0)
            e[r] = 0.5 if r % 2 == 0 else -1.0  # -1: on the inclusive clip boundary
            case.e = e
        y = ex.exact_targets(case)
        self.dataset = None
        if rows:
            g = torch.Generator(device="cpu").manual_seed(B)
            idx = torch.randperm(3 * B, generator=g)[:B]
            if variant[1] == "repeat":
                idx[5], idx[B - 1] = idx[100], idx[0]
            self.dataset = (case.x, y, idx)
            case = ex.ExactCase(case.lay, case.flat, case.x[idx], case.e[idx], case.grad_scale)
            y = y[idx]
        self.case, self.y = case, y
        self.lay, self.grad_scale = case.lay, case.grad_scale
        self.ref = ex.mlp_step_fp64(case.flat, case.x, y, case.grad_scale, loss, ex.CLIP, hidden=self.hidden)
        self.clip, self._violations = ex.CLIP, None

    def violations(self):
        from wellflow.train.exact import exactness_violations

        if self._violations is None:
            self._violations = exactness_violations(self.case, self.y, self.loss, self.clip)
        return self._violations

    @property
    def tag(self):
        return f"F={self.F} hidden={self.hidden} B={self.B} {self.loss} {self.variant or ''}"


@functools.lru_cache(maxsize=None)
def problem(F, hidden, B, loss, variant=None) -> Problem:
    return Problem(F, hidden, B, loss, variant)


def all_problem_keys():
    """Every (F, hidden, B, loss, variant) this file launches (the CPU file proves each exact)."""
    keys = []
    for loss in LOSSES:
        keys += [(F, HID, B, loss, None) for F in STEP_F for B in STEP_B]
        keys += [(F, HID, B, loss, None) for F in WIDE_F for B in WIDE_B]
        keys += [(F, HID, B, loss, None) for F in TAIL_F for B in TAIL_B]
        keys += [(OTHER_F, h, B, loss, None) for h in OTHER_HID for B in OTHER_B]
        keys += [(PROBE_F, HID, PROBE_B, loss, ("probe", r)) for r in PROBE_ROWS]
        keys += [(F, HID, CALL_B, loss, v) for F in CALL_F for v in (None, ("rows", "perm"), ("rows", "repeat"))]
        keys += [(F, HID, B, loss, None) for F in INFER_F for B in INFER_B]
    return list(dict.fromkeys(keys))


# ------------------------------------------------------------------ engines and comparison
_ENGINES = {}


def engine(F, loss, hidden=HID, env=()):
    """One engine per (F, loss, hidden, construction environment), reused across paths."""
    from wellflow.models.mlp import NativeMLP
    from wellflow.train.exact import CLIP

    key = (F, loss, tuple(hidden), tuple(sorted(dict(env).items())))
    if key not in _ENGINES:
        old = {k: os.environ.get(k) for k in dict(env)}
        os.environ.update(dict(env))
        try:
            _ENGINES[key] = NativeMLP(F, hidden, CAP, device=DEV, loss=loss, clip=CLIP)
        finally:
            for k, v in old.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
    return _ENGINES[key]


@contextlib.contextmanager
def switched(eng, **attrs):
    old = {k: getattr(eng, k) for k in attrs}
    try:
        for k, v in attrs.items():
            setattr(eng, k, v)
        yield eng
    finally:
        for k, v in old.items():
            setattr(eng, k, v)


def load(eng, prob) -> None:
    bad = prob.violations()
    assert not bad, f"{prob.tag}: the problem is not exact, nothing launched: {bad}"
    eng.params.copy_(prob.case.flat.float().to(DEV))
    eng.sync_weights()
    recompute = eng._recompute_ok(prob.B) and not eng.dw2_gemm
    if recompute:
        eng.Hs[0].fill_(float("nan"))  # a recompute step must neither read nor keep a stored H1
    eng.dZ[-1].fill_(float("nan"))    # every path writes dZ_L before it reads it


def _first_diff(got, want):
    ne = (got != want).reshape(-1)
    i = int(ne.nonzero()[0]) if bool(ne.any()) else -1
    return i, int(ne.sum())


def compare(eng, prob, ls, tag, mult: float = 1.0, loss_want=None) -> None:
    """pred, loss and the six gradient blocks == the float64 reference cast to fp32."""
    ref, B = prob.ref, prob.B
    torch.cuda.synchronize()
    got = {"pred": eng.pred[:B].cpu(), "loss": ls.detach().reshape(-1).cpu()}
    want = {"pred": ref["pred"].float(),
            "loss": (ref["loss_sum"] if loss_want is None else loss_want).reshape(-1).float()}
    gl, ghw, ghb = prob.lay.views(eng.grads.cpu())
    rl, rhw, rhb = prob.lay.views((ref["grads"] * mult).float())
    for l, ((gW, gb), (rW, rb)) in enumerate(zip(gl, rl)):
        got[f"dW{l + 1}"], want[f"dW{l + 1}"] = gW, rW  # padding columns included: exactly 0
        got[f"db{l + 1}"], want[f"db{l + 1}"] = gb, rb
    got["dw_head"], want["dw_head"], got["db_head"], want["db_head"] = ghw, rhw, ghb, rhb
    bad = []
    for name in got:
        if not torch.equal(got[name], want[name]):
            i, n = _first_diff(got[name], want[name])
            bad.append(f"{name}: {n} of {want[name].numel()} differ, first at flat index {i}: got "
                       f"{got[name].reshape(-1)[i].item()!r}, want {want[name].reshape(-1)[i].item()!r}")
    assert not bad, f"{tag} [{prob.tag}]\n  " + "\n  ".join(bad)
    if eng.red is not None:
        from wellflow.models.mlp import MLP_RED_COPY_FLOATS

        assert eng.red[:MLP_RED_COPY_FLOATS].abs().max().item() == 0.0, f"{tag}: scratch copies not re-zeroed"


def step(eng, prob, tag, **kw) -> None:
    load(eng, prob)
    x = prob.case.x.float().to(DEV)
    y = prob.y.float().to(DEV)
    ls = eng.forward_backward(x, y, prob.grad_scale, **kw)
    compare(eng, prob, ls, tag)


# ------------------------------------------------------------------ training-step paths
@pytest.mark.parametrize("F", STEP_F)
@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("path", list(STEP_PATHS))
def test_step_paths_exact(path, loss, F):
    """The eleven step paths at B = 64, 128, 192, 256 (the default 128-row one-launch step, its
    64-row form, row-major dZ2 + mlp2_dw2, the forward / backward pair, the pair with a stored
    H1 and the split-K dW2 GEMM, the stored-H1 step, GEMM backward, per-layer forward, H2 stored
    instead of its bitmask, direct atomics, and the 64-row step selected by the environment).
    Under mae_clip several fall back to the multi-launch path: only the result is asserted —
    which is what catches a path that silently trains on MSE (dw2_gemm did, before
    _recompute_ok sent it to the multi-launch path)."""
    attrs, env = STEP_PATHS[path]
    eng = engine(F, loss, env=tuple(env.items()))
    if path == "direct_atomics":
        assert eng.red is None
    elif path == "env_step64":
        assert eng.red is not None and eng.w2t is None
    else:
        assert eng.red is not None and eng.w2t is not None
    with switched(eng, **attrs):
        for B in STEP_B:
            step(eng, problem(F, HID, B, loss), path)
            assert eng._recompute_ok(B) == (path in H1_FREE[loss]), f"{path} {loss}: unexpected route"


@pytest.mark.parametrize("F", WIDE_F)
@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("path", ["default", "pair"])
def test_wide_features_exact(path, loss, F):
    """Fp = 40 .. 64: two 32-wide K tiles of W1 in the 128-row step; with the one-launch step
    switched off the multi-launch path computes dW1 as a split-K GEMM."""
    eng = engine(F, loss)
    with switched(eng, **STEP_PATHS[path][0]):
        for B in WIDE_B:
            assert eng._recompute_ok(B) == (path == "default")
            step(eng, problem(F, HID, B, loss), f"wide {path}")


@pytest.mark.parametrize("F", TAIL_F)
@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("path", ["default", "gemm_bwd"])
def test_batch_tails_exact(path, loss, F):
    """B % 64 != 0 at the (256, 256) shape: mlp2_forward / mlp2_backward with their row guards
    (the last batch of an epoch), and the head kernels + GEMMs with fused_bwd = False."""
    eng = engine(F, loss)
    with switched(eng, **STEP_PATHS[path][0]):
        for B in TAIL_B:
            assert not eng._recompute_ok(B)
            step(eng, problem(F, HID, B, loss), f"tail {path}")


@pytest.mark.parametrize("hidden", OTHER_HID)
@pytest.mark.parametrize("loss", LOSSES)
def test_other_hidden_shapes_exact(loss, hidden):
    """The per-layer path: GEMM + bias + ReLU epilogues, head kernels, dX GEMM with the mask and
    column-sum epilogue, split-K dW GEMMs; two hidden layers and one."""
    eng = engine(OTHER_F, loss, hidden=hidden)
    for B in OTHER_B:
        step(eng, problem(OTHER_F, hidden, B, loss), "per-layer")


@pytest.mark.parametrize("r", PROBE_ROWS)
@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("path", ["default", "pair"])
def test_single_live_row_exact(path, loss, r):
    """Only row r carries a gradient (first / last row of each 64-row chunk and 128-row pass):
    the six blocks equal that row's own float64 gradient and are nonzero, so a chunk edge that
    drops or doubles a row cannot hide in a sum over the batch."""
    from wellflow.train.exact import CLIP, mlp_step_fp64

    prob = problem(PROBE_F, HID, PROBE_B, loss, ("probe", r))
    one = mlp_step_fp64(prob.case.flat, prob.case.x[r : r + 1], prob.y[r : r + 1], prob.grad_scale, loss, CLIP)
    assert torch.equal(one["grads"], prob.ref["grads"])
    gl, ghw, ghb = prob.lay.views(one["grads"])
    for blk in (gl[0][0], gl[0][1], gl[1][0], gl[1][1], ghw, ghb):
        assert blk.abs().max().item() > 0
    eng = engine(PROBE_F, loss)
    with switched(eng, **STEP_PATHS[path][0]):
        step(eng, prob, f"probe row {r} {path}")


# ------------------------------------------------------------------ call shapes
@pytest.mark.parametrize("F", CALL_F)
@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("kind", ["perm", "repeat"])
@pytest.mark.parametrize("path", ["default", "pair", "gemm_bwd"])
def test_row_indexed_step_exact(path, kind, loss, F):
    """rows= over a 3B-row bf16 dataset in the input format: read through the index inside the
    fused kernels (default, pair) or gathered first (gemm_bwd); a permutation and an index that
    repeats rows."""
    prob = problem(F, HID, CALL_B, loss, ("rows", kind))
    X3, Y3, idx = prob.dataset
    eng = engine(F, loss)
    with switched(eng, **STEP_PATHS[path][0]):
        load(eng, prob)
        Xd = eng.to_input_format(X3.float().to(DEV))
        assert Xd.dtype == torch.bfloat16 and Xd.shape == (3 * CALL_B, eng.Fp)
        ls = eng.forward_backward(Xd, Y3.float().to(DEV), prob.grad_scale, rows=idx.to(DEV))
        compare(eng, prob, ls, f"rows {kind} {path}")


@pytest.mark.parametrize("F", CALL_F)
@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("path", ["default", "pair", "gemm_bwd"])
def test_accumulating_calls_exact(path, loss, F):
    """zero_grads=False twice = exactly twice the gradient; loss_into= adds exactly; three
    steps in a row give identical results and leave the scratch copies zeroed."""
    prob = problem(F, HID, CALL_B, loss)
    eng = engine(F, loss)
    x, y = prob.case.x.float().to(DEV), prob.y.float().to(DEV)
    L = prob.ref["loss_sum"]
    with switched(eng, **STEP_PATHS[path][0]):
        load(eng, prob)
        ls = eng.forward_backward(x, y, prob.grad_scale)
        compare(eng, prob, ls, f"{path} first")
        ls = eng.forward_backward(x, y, prob.grad_scale, zero_grads=False)
        compare(eng, prob, ls, f"{path} accumulated", mult=2.0)
        acc = torch.full((1,), 3.0, device=DEV)
        for k in (1, 2):
            out = eng.forward_backward(x, y, prob.grad_scale, loss_into=acc)
            assert out is acc
            compare(eng, prob, acc, f"{path} loss_into {k}", loss_want=3.0 + k * L)
        for k in range(3):
            ls = eng.forward_backward(x, y, prob.grad_scale)
            compare(eng, prob, ls, f"{path} repeat {k}")


# ------------------------------------------------------------------ inference
@pytest.mark.parametrize("F", INFER_F)
@pytest.mark.parametrize("route", ["fp32_F", "fp32_Fp", "bf16_inplace", "bf16_view", "per_layer"])
def test_forward_exact(route, F):
    """forward() through every _load_x route: fp32 [B][F] (transpose_cast_bf16 when F % 8 != 0),
    fp32 [B][Fp] (cast_bf16), bf16 in the input format read in place, bf16 from a
    non-contiguous view (copied), and the per-layer GEMMs + head_fwd."""
    eng = engine(F, "mse")
    Fp = eng.Fp
    with switched(eng, fused=route != "per_layer"):
        for B in INFER_B:
            prob = problem(F, HID, B, "mse")
            load(eng, prob)
            xp = torch.zeros(B, Fp)
            xp[:, :F] = prob.case.x.float()
            if route in ("fp32_F", "per_layer"):
                xin = prob.case.x.float().to(DEV)
            elif route == "fp32_Fp":
                xin = xp.to(DEV)
            elif route == "bf16_inplace":
                xin = xp.to(DEV).to(torch.bfloat16)
                assert xin.is_contiguous() and xin.data_ptr() % 16 == 0
            else:
                big = torch.full((B, Fp + 8), 7.0, dtype=torch.bfloat16, device=DEV)
                big[:, 8:] = xp.to(DEV).to(torch.bfloat16)
                xin = big[:, 8:]
                assert B == 1 or not xin.is_contiguous()
            eng.pred.fill_(float("nan"))
            got = eng.forward(xin)
            torch.cuda.synchronize()
            want = prob.ref["pred"].float()
            if not torch.equal(got.cpu(), want):
                i, n = _first_diff(got.cpu(), want)
                raise AssertionError(f"forward {route} [{prob.tag}]: {n} of {B} differ, first at row {i}: got "
                                     f"{got[i].item()!r}, want {want[i].item()!r}")


# ------------------------------------------------------------------ host-side refusal
def test_fused_steps_refuses_unpadded_rows():
    """fused_steps reads rows with stride Fp: a bf16 [N][5] tensor (Fp = 8) that did not go
    through to_input_format is refused on the host, before the scratch is allocated or anything
    is launched."""
    from wellflow.models.mlp import NativeMLP
    from wellflow.optim.flat import FlatAdam

    F, B = 5, 64
    eng = NativeMLP(F, HID, B, device=DEV)
    prob = problem(F, HID, 64, "mse")
    eng.params.copy_(prob.case.flat.float().to(DEV))
    eng.sync_weights()
    opt = FlatAdam(eng.params, eng.grads, lr=1e-3, shadow=eng.shadow, zero_grads=True, shadow_t=eng.shadow_t)
    X = prob.case.x.to(torch.bfloat16).to(DEV)
    Y = prob.y.float().to(DEV)
    assert X.shape == (B, F) and eng.Fp == 8
    assert eng.small_steps_reason(B, opt, X) is None  # everything but the row width is acceptable
    p0, t0 = eng.params.clone(), opt.t
    for bad in (X, eng.to_input_format(X).reshape(-1)):
        with pytest.raises(RuntimeError, match=r"X must be \[N\]\[8\]"):
            eng.fused_steps(bad, Y, B, 1, opt, 1.0 / B)
    torch.cuda.synchronize()
    assert eng.small.scratch is None and eng.small.sync is None and opt.t == t0 and torch.equal(eng.params, p0)
    eng.fused_steps(eng.to_input_format(X), Y, B, 1, opt, 1.0 / B)  # the input format is accepted
    torch.cuda.synchronize()
    eng.check_device_errors()
    assert opt.t == t0 + 1 and math.isfinite(eng.params.sum().item()) and not torch.equal(eng.params, p0)
