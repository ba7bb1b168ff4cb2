"""mlp_small_kernel (csrc/mlp_small.hip, NativeMLP.fused_steps) against the float64 step, element
by element.

The batches come from wellflow/train/exact.py, where bf16 / fp32 arithmetic never rounds, so the
gradient the kernel forms inside the launch must equal the float64 one bit for bit. It is never
stored, but Adam's first step from zero state shows it: ``m = fl(fl(1 - b1) g)`` and ``v =
fl(fl(fl(1 - b2) g) g)`` have one fp32 answer (optim_ref.adam_moments_fp32), asserted with
``torch.equal`` on every element of every block. The parameters are held to the derived bound of
``sb_adam`` (optim_ref.adam_p_tol, form "hw").

K steps in one launch are pinned with the parameters held still (lr = 0, betas 0.5): the first
moment is then the exact dyadic sum of the K float64 gradients, so a row misread in step k > 0,
a stale prefetch or a stale granule changes bits of ``m``.

tests/test_optim_exact_cpu.py proves every slice exact without a GPU.
Worst measured error / bound on an MI355X: one step p 0.340, v 0.446, m 0.317 (and m, v equal the
fp32 moments bit for bit); K steps v 0.335.
"""
import functools

import pytest
import torch

from wellflow.train import exact as ex
from wellflow.train import optim_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
NAN = float("nan")

HID = (256, 256)
LOSSES = ("mse", "mae_clip")
ONE_F, ONE_B = (5, 16, 24, 32), (32, 96, 256)  # Fp = 8, 16 (NFT = 1) and 24, 32 (NFT = 2)
ONE_WD, ONE_LAYOUTS = (0.0, 0.01), ("contiguous", "rows")
ONE_LR = 1e-3
ONE_HP = {wd: dict(b1=0.9, b2=0.999, eps=1e-8, wd=wd, gscale=1.0, clip=None, cv=False, lattice=False) for wd in ONE_WD}
K_STEPS, K_F, K_B = 3, (5, 24), (96, 256)
K_T0 = (0, 4094, 4097)  # three launches on one engine: fresh, from a preset counter, continuing
LOSS_ACC0 = 3.0


def seed_for(F, B, layout):
    return 1000 * F + B + (500 if layout == "rows" else 0)


class Batches:
    """One exact_mlp_case of N rows (one set of lattice weights) and its per-step slices."""

    def __init__(self, F, B, loss, steps, layout):
        self.F, self.B, self.loss, self.steps, self.layout = F, B, loss, steps, layout
        N = steps * B * (3 if layout == "rows" and steps == 1 else 1)
        case = ex.exact_mlp_case(F, HID, N, seed_for(F, B, layout))
        case.grad_scale = ex.exact_grad_scale(B)
        self.case, self.lay, self.grad_scale = case, case.lay, case.grad_scale
        self.y = ex.exact_targets(case)
        if layout == "rows":
            self.rows = torch.randperm(N, generator=torch.Generator().manual_seed(B + F))[: steps * B]
        else:
            self.rows = torch.arange(steps * B)
        self.slices, self.refs = [], []
        for k in range(steps):
            idx = self.rows[k * B: (k + 1) * B]
            sl = ex.ExactCase(case.lay, case.flat, case.x[idx], case.e[idx], case.grad_scale)
            self.slices.append((sl, self.y[idx]))
            self.refs.append(ex.mlp_step_fp64(case.flat, sl.x, self.y[idx], case.grad_scale, loss, ex.CLIP, hidden=HID))

    def violations(self):
        bad = []
        for k, (sl, y) in enumerate(self.slices):
            bad += [f"step {k}: {b}" for b in ex.exactness_violations(sl, y, self.loss, ex.CLIP)]
        return bad

    @property
    def tag(self):
        return f"F={self.F} B={self.B} {self.loss} {self.layout} steps={self.steps}"


@functools.lru_cache(maxsize=None)
def batches(F, B, loss, steps, layout) -> Batches:
    return Batches(F, B, loss, steps, layout)


def one_step_keys():
    return [(F, B, loss, 1, lay) for F in ONE_F for B in ONE_B for loss in LOSSES for lay in ONE_LAYOUTS]


def k_step_keys():
    return [(F, B, loss, K_STEPS, "rows") for F in K_F for B in K_B for loss in LOSSES]


def k_step_moments(bt: Batches, m0, v0):
    """(m, v, bound of v) after the K steps with betas (0.5, 0.5), float64: m = sum_k 2^-(K-k+1)
    g_k + 2^-K m0 (every term dyadic: exact in fp32, asserted on the CPU); v's error obeys
    e_k = e_{k-1} / 2 + adam_v_tol(v_k)."""
    m, v = m0.double(), v0.double()
    e = torch.zeros_like(v)
    for ref in bt.refs:
        g = ref["grads"]
        m = 0.5 * m + 0.5 * g
        v = 0.5 * v + 0.5 * g * g
        e = 0.5 * e + R.adam_v_tol(v)
    return m, v, e


# ------------------------------------------------------------------------------ device side
_ENGINES = {}


def engine(F, loss):
    from wellflow.models.mlp import NativeMLP

    if (F, loss) not in _ENGINES:
        _ENGINES[(F, loss)] = NativeMLP(F, HID, 256, device=DEV, loss=loss, clip=ex.CLIP)
    return _ENGINES[(F, loss)]


def _optimizer(eng, lr, betas, wd):
    from wellflow.optim.flat import FlatAdam

    return FlatAdam(eng.params, eng.grads, lr=lr, betas=betas, weight_decay=wd, shadow=eng.shadow, zero_grads=True,
                    shadow_t=eng.shadow_t)


def _launch(eng, opt, bt, K, acc):
    """Parameters loaded, every output the launch must write prefilled with NaN, the gradient
    bucket with a sentinel; returns after the launch has completed without a device error."""
    assert not bt.violations(), f"{bt.tag}: the batches are not exact, nothing launched"
    eng.params.copy_(bt.case.flat.float().to(DEV))
    eng.shadow.fill_(NAN)
    if eng.w2t is not None:
        eng.w2t.fill_(NAN)
    eng.grads.fill_(7.0)
    if bt.layout == "rows":
        X, Y, rows = bt.case.x, bt.y, bt.rows.to(DEV)
    else:
        X, Y, rows = bt.case.x, bt.y, None
    Xd = eng.to_input_format(X.float().to(DEV))
    assert Xd.dtype == BF and Xd.shape[1] == eng.Fp
    eng.fused_steps(Xd, Y.float().to(DEV), bt.B, K, opt, bt.grad_scale, rows=rows, loss_into=acc)
    torch.cuda.synchronize()
    eng.check_device_errors()


def _images_and_bucket(eng, bt):
    """shadow / W2^T = bf16 of the device's own new parameters on every block (the layout's
    padding words are not the kernel's to write: still NaN); the gradient bucket untouched."""
    offs, hw, hb, n = bt.lay.offsets()
    block = torch.zeros(n, dtype=torch.bool)
    for (w, b), (h, k) in zip(offs, bt.lay.dims):
        block[w: w + h * k] = True
        block[b: b + h] = True
    block[hw: hw + HID[-1]] = True
    block[hb] = True
    sh, p = eng.shadow.cpu(), eng.params.cpu()
    assert torch.equal(sh[block], p.to(BF)[block]), "shadow != bf16 of the new parameters"
    assert bool(sh[~block].isnan().all()), "shadow written outside the parameter blocks"
    if eng.w2t is not None:
        w2 = offs[1][0]
        want = eng.params[w2: w2 + 65536].view(256, 256).t().contiguous().to(BF).view(-1)
        assert torch.equal(eng.w2t, want), "W2^T image != bf16 of the new W2, transposed"
    assert bool((eng.grads == 7.0).all()), "the gradient bucket was written"


def _counter(opt, want):
    assert opt.step_dev[0].item() == float(want) and opt.t == want
    assert opt.step_dev[1:2].view(torch.int32).item() == 0


def _adam_violations():
    """adam_violations of tests/test_optim_exact_gpu.py (the comparator the CPU file proves)."""
    import importlib.util
    import os

    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_optim_exact_gpu.py")
    spec = importlib.util.spec_from_file_location("_optim_exact_gpu_cmp", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.adam_violations


@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("F", ONE_F)
def test_small_one_step_matches_fp64(F, loss):
    """K = 1 at B = 32, 96, 256, contiguous rows and a permutation into a 3 B-row table, wd 0 and
    0.01: m, v bit for bit the fp32 moments of the float64 gradient, the parameters inside the
    sb_adam bound, untouched where g = 0 (W1's padding columns too), the loss sum added exactly,
    images from NaN prefill, counter, bucket. Worst measured error / bound: p 0.340 (the bias
    corrections carry optim_ref.DELTA_POWF, measured through adam_dev_kernel's identical __powf)."""
    check = _adam_violations()
    eng = engine(F, loss)
    ratios = {}
    for B in ONE_B:
        for layout in ONE_LAYOUTS:
            bt = batches(F, B, loss, 1, layout)
            ref = bt.refs[0]
            for wd in ONE_WD:
                opt = _optimizer(eng, ONE_LR, (0.9, 0.999), wd)
                acc = torch.full((1,), LOSS_ACC0, device=DEV)
                _launch(eng, opt, bt, 1, acc)
                p0 = bt.case.flat.float()
                zero = torch.zeros_like(p0)
                g = ref["grads"].float()
                assert torch.equal(g.double(), ref["grads"])
                got = (eng.params.cpu(), opt.m.cpu(), opt.v.cpu())
                bad = check(got, (p0, zero, zero), g, ONE_HP[wd], 0.0, 1, form="hw", lr=ONE_LR, ratios=ratios)
                assert not bad, f"mlp_small {bt.tag} wd={wd}\n  " + "\n  ".join(bad)
                assert acc.item() == float(LOSS_ACC0 + ref["loss_sum"]), (acc.item(), float(ref["loss_sum"]))
                _counter(opt, 1)
                _images_and_bucket(eng, bt)
    print("[ratio] mlp_small one step " + " ".join(f"{k}={r:.3f}" for k, r in sorted(ratios.items())))


@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("B", K_B)
@pytest.mark.parametrize("F", K_F)
def test_small_k_steps_parameters_held_still(F, B, loss):
    """K = 3 distinct batches in one launch with lr = 0, wd = 0, betas (0.5, 0.5): parameters
    bit-unchanged, m bit for bit the dyadic sum of the three float64 gradients, v inside its
    bound, the loss sum exact, counter + K. Three launches on one engine: from zero, from a counter
    preset to 4094 (zero moments again), and continuing from that launch's moments — the granule
    tags and the W2^T parity buffers past their first use. Worst measured v error / bound: 0.335."""
    eng = engine(F, loss)
    bt = batches(F, B, loss, K_STEPS, "rows")
    opt = _optimizer(eng, 0.0, (0.5, 0.5), 0.0)
    p0 = bt.case.flat.float()
    loss_total = sum(ref["loss_sum"] for ref in bt.refs)
    worst = 0.0
    for t0 in K_T0:
        if t0 != K_T0[2]:  # the third launch continues from the second's moments and counter
            opt.m.zero_()
            opt.v.zero_()
            opt.step_dev.zero_()
            opt.step_dev[0] = float(t0)
            opt.t = t0
        m0, v0 = opt.m.cpu(), opt.v.cpu()
        acc = torch.full((1,), LOSS_ACC0, device=DEV)
        _launch(eng, opt, bt, K_STEPS, acc)
        m, v, e = k_step_moments(bt, m0, v0)
        tag = f"mlp_small {bt.tag} from t={t0}"
        assert torch.equal(eng.params.cpu(), p0), f"{tag}: parameters moved with lr = 0"
        gm = opt.m.cpu().double()
        if not torch.equal(gm, m):
            i = int((gm != m).nonzero()[0])
            raise AssertionError(f"{tag}: m differs on {int((gm != m).sum())} of {m.numel()} elements, first at {i}: "
                                 f"got {gm[i].item()!r}, want {m[i].item()!r}")
        err = (opt.v.cpu().double() - v).abs()
        assert bool((err <= e).all()), f"{tag}: v outside its bound at {int((~(err <= e)).nonzero()[0])}"
        worst = max(worst, float(torch.where(err == 0, err, err / e).max()))
        assert acc.item() == float(LOSS_ACC0 + loss_total), (acc.item(), float(loss_total))
        _counter(opt, t0 + K_STEPS)
        _images_and_bucket(eng, bt)
    print(f"[ratio] mlp_small K steps v={worst:.3f}")
