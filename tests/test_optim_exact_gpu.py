"""The Adam and SGD update kernels (csrc/elementwise.hip: adam_kernel, adam_dev_kernel,
lstm_adam_pack_kernel, sgd_kernel, sgd_dev_kernel) against the float64 rules of
wellflow/train/optim_ref.py, element by element, one step at a time.

Every step is compared with the reference fed the device's own state before that step (fp32
widened to float64), so nothing accumulates. Tolerances are the derived bounds of optim_ref.py
plus one measured number, ``DELTA_POWF`` (the error of ``__powf`` in the bias corrections,
re-measured by ``test_powf_error_is_within_delta``); the moments are also held bit for bit from
zero state (``adam_moments_fp32``) and on a dyadic lattice with b1 = b2 = 0.5. No comparator
masks an element.

The input sets and the comparators below are imported by tests/test_optim_exact_cpu.py, which
proves without a GPU that they reject every planted error of its list at these tolerances.

Measured on an MI355X (worst |error| / bound over every element of every case; the bounds end
in half an ulp of the result, which some element of a large case nearly reaches):
adam_dev_kernel p 0.996, m 0.616, v 0.491; adam_kernel p 0.982, m 0.635, v 0.491;
lstm_adam_pack_kernel p 0.997, m 0.630, v 0.535; sgd_dev_kernel p 0.928, vel 0.931; sgd_kernel
p 0.779, vel 0.728; 0 on the lattices. Worst measured __powf error 1.68e-7 (DELTA_POWF 3.4e-7).
"""
import functools
import itertools

import pytest
import torch

from wellflow.train import optim_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
NAN = float("nan")

# ------------------------------------------------------------------------------ the input sets
ADAM_N = (1, 3, 4, 5, 1023, 1025, 262149)  # 262,149: one past 256 workgroups x 256 lanes x 4
ADAM_T0 = (0, 1, 9, 999, 99999)            # the device counter before the step (t = T0 + 1)
ADAM_LR = 0.05
STEPS = 3
# name -> b1, b2, eps, wd, gscale, clip factor preset in the state block (None: no block),
# clipvalue bites (a value some |g gs| equal exactly), inputs on the dyadic lattice
ADAM_HP = {
    "default":      dict(b1=0.9, b2=0.999, eps=1e-8, wd=0.0, gscale=1.0, clip=None, cv=False, lattice=False),
    "wd_gs_clip":   dict(b1=0.9, b2=0.999, eps=1e-8, wd=0.01, gscale=1 / 64, clip=0.25, cv=True, lattice=False),
    "wd_gs":        dict(b1=0.9, b2=0.999, eps=1e-8, wd=0.01, gscale=1 / 64, clip=None, cv=False, lattice=False),
    "half_wd_cv":   dict(b1=0.5, b2=0.5, eps=1e-3, wd=0.01, gscale=1.0, clip=None, cv=True, lattice=True),
    "half_gs_clip": dict(b1=0.5, b2=0.5, eps=1e-3, wd=0.0, gscale=1 / 64, clip=0.25, cv=False, lattice=True),
    "half_wd_gs":   dict(b1=0.5, b2=0.5, eps=1e-3, wd=0.01, gscale=1 / 64, clip=None, cv=False, lattice=True),
}
ADAM_PLAIN_HP = ("default", "wd_gs", "half_wd_gs")  # adam_kernel has no clipping arguments
ADAM_BIG_HP = ("default", "wd_gs_clip")             # at n = 262,149 (the stride is what that size is for)
LATTICE_CV = 0.5

SGD_N = (1, 255, 257, 524289)  # 524,289: one past 2048 workgroups x 256 lanes
SGD_IT0 = (0, 1, 10 ** 6)
SGD_HP = {
    # the lattice of test_cnn_exact_gpu.py::test_cnn_sgd_pack_matches_fp64_keras_step
    "lattice":       dict(lr=0.25, mu=0.5, decay=0.0, gscale=0.5, clip=None, cv=False, lattice=True),
    "lattice_clip":  dict(lr=0.25, mu=0.5, decay=0.0, gscale=0.5, clip=0.25, cv=True, lattice=True),
    "decay":         dict(lr=0.1, mu=0.9, decay=1e-6, gscale=1.0, clip=None, cv=False, lattice=False),
    "decay_gs_clip": dict(lr=0.1, mu=0.9, decay=1e-6, gscale=1 / 64, clip=0.25, cv=True, lattice=False),
}
SGD_PLAIN_HP = ("lattice", "decay")
SGD_BIG_HP = ("lattice", "decay_gs_clip")


def adam_cases():
    return [(n, h) for n in ADAM_N for h in ADAM_HP if n < 100000 or h in ADAM_BIG_HP]


def sgd_cases():
    return [(n, h, nes) for n in SGD_N for h in SGD_HP for nes in (True, False) if n < 100000 or h in SGD_BIG_HP]


def _pick(values, n, g):
    v = torch.tensor(values, dtype=torch.float32)
    return v[torch.randint(0, len(values), (n,), generator=g)]


def _kinds(n):
    """Per element: 0 ordinary, 1 tiny gradients (1e-4: eps matters), 2 dead (g = m = v = 0 on
    every step: the parameter may move only by weight decay)."""
    i = torch.arange(n)
    k = torch.zeros(n, dtype=torch.long)
    k[i % 10 == 3] = 1
    k[i % 10 == 7] = 2
    return k


def _scale_of(hp):
    return R.f32(hp["gscale"]) * (1.0 if hp["clip"] is None else hp["clip"])


@functools.lru_cache(maxsize=None)
def adam_inputs(n, hpname, start):
    """p0, m0, v0 (fp32), the raw gradients of the three steps and the clipvalue. The EFFECTIVE
    gradients are drawn first and divided by the (power of two) scale, so the scaling is exact."""
    hp = ADAM_HP[hpname]
    g = torch.Generator().manual_seed(1000 * n + 7 * sorted(ADAM_HP).index(hpname) + (start == "nonzero"))
    kinds = _kinds(n)
    dead = kinds == 2
    p0 = 0.1 * torch.randn(n, generator=g)
    ges = []
    for _ in range(STEPS):
        if hp["lattice"]:
            ge = _pick((-1.5, -1.0, -0.5, -0.125, -0.03125, 0.03125, 0.125, 0.5, 1.0, 1.5), n, g)
        else:
            ge = torch.randn(n, generator=g)
            ge[kinds == 1] *= 1e-4
        ge[dead] = 0.0
        ges.append(ge)
    if start == "zero":
        m0, v0 = torch.zeros(n), torch.zeros(n)
    elif hp["lattice"]:
        m0, v0 = _pick((-0.5, -0.25, 0.0, 0.25, 0.5), n, g), _pick((0.0, 0.0625, 0.25, 1.0, 3.0), n, g)
    else:
        m0, v0 = 0.1 * torch.randn(n, generator=g), 0.01 * torch.randn(n, generator=g) ** 2
        m0[kinds == 1] *= 1e-4  # the tiny elements stay at the scale of eps
        v0[kinds == 1] *= 1e-8
    m0[dead], v0[dead] = 0.0, 0.0
    cv = 0.0
    if hp["cv"]:
        live = ges[0][~dead].abs()
        cv = LATTICE_CV if hp["lattice"] else (float(live.median()) if live.numel() else 0.5)  # median: an element's own value
    scale = _scale_of(hp)
    assert R.is_pow2(scale)
    return p0, m0, v0, tuple(ge / scale for ge in ges), cv


@functools.lru_cache(maxsize=None)
def sgd_inputs(n, hpname):
    hp = SGD_HP[hpname]
    g = torch.Generator().manual_seed(77 * n + sorted(SGD_HP).index(hpname))
    scale = _scale_of(hp)
    assert R.is_pow2(scale)
    if hp["lattice"]:
        p0 = _pick(tuple(k / 8 for k in range(-15, 16)), n, g)
        vel0 = _pick((-0.5, 0.0, 0.5), n, g)
        # the CNN test's lattice: effective gradients on {-2, -1, 0, 1, 2} (the raw ones scaled up by
        # the preset factor); with the clamp at 1 also +-1/2, so that some elements lie inside it
        vals = (-2.0, -1.0, -0.5, 0.0, 0.5, 1.0, 2.0) if hp["cv"] else (-2.0, -1.0, 0.0, 1.0, 2.0)
        ges = [_pick(vals, n, g) for _ in range(STEPS)]
        cv = 1.0 if hp["cv"] else 0.0
    else:
        p0 = 0.01 * torch.randn(n, generator=g)
        vel0 = 0.01 * torch.randn(n, generator=g)
        ges = [torch.randn(n, generator=g) for _ in range(STEPS)]
        cv = float(ges[0].abs().median()) if hp["cv"] else 0.0
    return p0, vel0, tuple(ge / scale for ge in ges), cv


# ------------------------------------------------------------------------------ the comparators
def _worst(err, tol):
    """max error / tolerance with 0 / 0 = 0 (an exact element of zero tolerance) and x / 0 = inf."""
    r = torch.where(err == 0, torch.zeros_like(err), err / tol)
    return float(r.max()) if r.numel() else 0.0


def _within(name, got, want, tol, bad, ratios):
    err = (got.double() - want).abs()
    ok = err <= tol  # False for NaN
    ratios[name] = max(ratios.get(name, 0.0), _worst(err, tol))
    if not bool(ok.all()):
        i = int((~ok).nonzero()[0])
        bad.append(f"{name}: {int((~ok).sum())} of {ok.numel()} outside the bound, first at {i}: got "
                   f"{got[i].item()!r}, want {want[i].item()!r}, bound {tol[i].item():.3g}")


def _equal(name, got, want, bad):
    same = (got == want) | (got.isnan() & want.isnan())
    if got.shape != want.shape or not bool(same.all()):
        i = int((~same).reshape(-1).nonzero()[0])
        bad.append(f"{name}: {int((~same).sum())} of {want.numel()} differ, first at {i}: got "
                   f"{got.reshape(-1)[i].item()!r}, want {want.reshape(-1)[i].item()!r}")


def adam_violations(got, before, g_raw, hp, cv, t, form="ieee", delta=R.DELTA_POWF, lr=ADAM_LR, ratios=None):
    """Why (p, m, v) = ``got`` is not one Adam step ``t`` of ``before`` = (p, m, v) on ``g_raw``:
    an empty list when every element is inside its bound. ``ratios`` collects error / bound."""
    bad, ratios = [], ({} if ratios is None else ratios)
    p0, m0, v0 = before
    b1, b2, eps, wd = (R.f32(hp[k]) for k in ("b1", "b2", "eps", "wd"))
    lr32 = R.f32(lr)
    fac = 1.0 if hp["clip"] is None else hp["clip"]
    pn, mn, vn = R.adam_fp64(p0, g_raw, m0, v0, t, lr32, b1, b2, eps, wd, R.f32(hp["gscale"]), fac, cv)
    ge32 = R.effective_grad_fp32(g_raw, hp["gscale"], hp["clip"], cv)
    ge = R.effective_grad_fp64(g_raw, R.f32(hp["gscale"]), fac, cv)
    g_rel = R.grad_rel_error(hp["gscale"], hp["clip"])
    if g_rel == 0.0:
        assert torch.equal(ge32.double(), ge)
    _within("m", got[1], mn, R.adam_m_tol(ge, m0, b1, g_rel), bad, ratios)
    _within("v", got[2], vn, R.adam_v_tol(vn, g_rel), bad, ratios)
    _within("p", got[0], pn, R.adam_p_tol(p0, ge, m0, mn, vn, pn, t, lr32, b1, b2, eps, wd, delta, form, g_rel),
            bad, ratios)
    if not bool(m0.any()) and not bool(v0.any()):  # from zero state: fp32 has one answer
        m32, v32 = R.adam_moments_fp32(ge32, b1, b2)
        _equal("m from zero state", got[1], m32, bad)
        _equal("v from zero state", got[2], v32, bad)
    if hp["lattice"]:  # b = 0.5 on dyadic values: no operation rounds
        _equal("m on the lattice", got[1].double(), mn, bad)
        _equal("v on the lattice", got[2].double(), vn, bad)
    if wd == 0.0:
        still = (ge == 0) & (m0 == 0) & (v0 == 0)
        _equal("p where g = m = v = 0", got[0][still], p0[still], bad)
    return bad


def sgd_violations(got, before, g_raw, hp, cv, it, nesterov, host_lr=False, ratios=None):
    bad, ratios = [], ({} if ratios is None else ratios)
    p0, vel0 = before
    lr, mu, decay = (R.f32(hp[k]) for k in ("lr", "mu", "decay"))  # host_lr (sgd_kernel): lr_t arrives rounded to fp32
    fac = 1.0 if hp["clip"] is None else hp["clip"]
    pn, vn = R.sgd_fp64(p0, g_raw, vel0, it, lr, mu, nesterov, decay, R.f32(hp["gscale"]), fac, cv)
    ge = R.effective_grad_fp64(g_raw, R.f32(hp["gscale"]), fac, cv)
    g_rel = R.grad_rel_error(hp["gscale"], hp["clip"])
    e_p, e_v = R.sgd_tol(pn, ge, vel0, vn, it, lr, mu, nesterov, decay, g_rel, host_lr)
    _within("vel", got[1], vn, e_v, bad, ratios)
    _within("p", got[0], pn, e_p, bad, ratios)
    if hp["lattice"]:
        _equal("vel on the lattice", got[1].double(), vn, bad)
        _equal("p on the lattice", got[0].double(), pn, bad)
    return bad


# ------------------------------------------------------------------------------ device helpers
def _lib():
    from wellflow.ops.native import lib

    return lib()


def _clip_block(factor):
    """The state block as grad_clip_scale_kernel leaves it, written by the test: no norm launch."""
    if factor is None:
        return None
    st = torch.zeros(8, device=DEV)
    st[0] = factor
    return st


def _counter(step, want):
    assert step[0].item() == float(want), f"step counter {step[0].item()} != {want}"
    assert step[1:2].view(torch.int32).item() == 0, "ticket word not returned to zero"


def _note(kernel, ratios):
    """The measured figures (pytest -s): worst error / bound per quantity of this case."""
    print(f"[ratio] {kernel} " + " ".join(f"{k}={r:.3f}" for k, r in sorted(ratios.items())))


# ------------------------------------------------------------------------------ Adam
@pytest.mark.parametrize("n,hpname", adam_cases())
def test_adam_dev_matches_fp64(n, hpname):
    """adam_dev_kernel: every counter preset x zero / non-zero starting moments, three steps with
    a new gradient each; shadow from NaN prefill, the bucket cleared or kept, counter and ticket.
    Worst measured error / bound: p 0.996, m 0.616, v 0.491 (DELTA_POWF 3.4e-7 from 1.68e-7 measured)."""
    C, hp = _lib(), ADAM_HP[hpname]
    ratios = {}
    for (t0, start), zero_g in zip(itertools.product(ADAM_T0, ("zero", "nonzero")), itertools.cycle((True, False))):
        p0, m0, v0, grads, cv = adam_inputs(n, hpname, start)
        p, m, v = p0.to(DEV), m0.to(DEV), v0.to(DEV)
        step = torch.zeros(4, device=DEV)
        step[0] = float(t0)
        clip = _clip_block(hp["clip"])
        for k, g_raw in enumerate(grads):
            before = (p.cpu(), m.cpu(), v.cpu())
            g = g_raw.to(DEV)
            shadow = torch.full((n,), NAN, dtype=BF, device=DEV)
            C.adam_dev(p, g, m, v, step, ADAM_LR, hp["b1"], hp["b2"], hp["eps"], hp["wd"], hp["gscale"], shadow,
                       zero_g, None, 0, 0, 0, clip, cv)
            torch.cuda.synchronize()
            t = t0 + k + 1
            bad = adam_violations((p.cpu(), m.cpu(), v.cpu()), before, g_raw, hp, cv, t, ratios=ratios)
            assert not bad, f"adam_dev n={n} {hpname} t={t} start={start}\n  " + "\n  ".join(bad)
            _counter(step, t)
            assert torch.equal(g.cpu(), torch.zeros(n) if zero_g else g_raw), "bucket not cleared / not kept"
            assert torch.equal(shadow, p.to(BF)), "shadow != bf16 of the new parameters"
            if clip is not None:
                assert clip[0].item() == hp["clip"] and clip[1:].abs().max().item() == 0.0
    _note("adam_dev", ratios)


@pytest.mark.parametrize("n,hpname", [(n, h) for n, h in adam_cases() if h in ADAM_PLAIN_HP])
def test_adam_host_corrections_matches_fp64(n, hpname):
    """adam_kernel (bias corrections from the host, rounded to fp32: DELTA = 0 in the bound).
    Worst measured error / bound: p 0.982, m 0.635, v 0.491."""
    C, hp = _lib(), ADAM_HP[hpname]
    ratios = {}
    b1, b2 = R.f32(hp["b1"]), R.f32(hp["b2"])
    for t0, start in itertools.product(ADAM_T0, ("zero", "nonzero")):
        p0, m0, v0, grads, cv = adam_inputs(n, hpname, start)
        p, m, v = p0.to(DEV), m0.to(DEV), v0.to(DEV)
        for k, g_raw in enumerate(grads):
            before = (p.cpu(), m.cpu(), v.cpu())
            g = g_raw.to(DEV)
            t = t0 + k + 1
            C.adam(p, g, m, v, ADAM_LR, hp["b1"], hp["b2"], hp["eps"], hp["wd"], 1.0 - b1 ** t, 1.0 - b2 ** t,
                   hp["gscale"])
            torch.cuda.synchronize()
            bad = adam_violations((p.cpu(), m.cpu(), v.cpu()), before, g_raw, hp, cv, t, delta=0.0, ratios=ratios)
            assert not bad, f"adam n={n} {hpname} t={t} start={start}\n  " + "\n  ".join(bad)
            assert torch.equal(g.cpu(), g_raw)
    _note("adam", ratios)


# shadow_t placements: (n, t_off, rows, cols)
SHADOW_T = [
    (1027, 0, 8, 16),       # t_off = 0
    (1027, 7, 8, 16),       # off a float4 boundary at both ends
    (1027, 1018, 3, 3),     # straddles the float4 body (1024 elements) / scalar tail boundary, ends at n - 1
    (1024, 1000, 4, 6),     # ends at n - 1 inside the float4 body
    (1027, 5, 1, 37),       # 1 x c
    (1027, 1022, 5, 1),     # r x 1, ends at n - 1
    (3, 1, 2, 1),           # no float4 body at all
]


@pytest.mark.parametrize("n,t_off,rows,cols", SHADOW_T)
def test_adam_dev_shadow_t_block(n, t_off, rows, cols):
    """The transposed bf16 block: exactly the [rows][cols] block at t_off, transposed, and not an
    element outside it (the destination sits inside a larger NaN-filled buffer)."""
    C, hp = _lib(), ADAM_HP["default"]
    g0 = torch.Generator().manual_seed(n + t_off)
    p = torch.randn(n, generator=g0).to(DEV)
    g = torch.randn(n, generator=g0).to(DEV)
    m, v = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    step = torch.zeros(4, device=DEV)
    pad = 64
    buf = torch.full((pad + rows * cols + pad,), NAN, dtype=BF, device=DEV)
    shadow = torch.full((n,), NAN, dtype=BF, device=DEV)
    C.adam_dev(p, g, m, v, step, ADAM_LR, hp["b1"], hp["b2"], hp["eps"], 0.0, 1.0, shadow, False,
               buf[pad: pad + rows * cols], t_off, rows, cols, None, 0.0)
    torch.cuda.synchronize()
    _counter(step, 1)
    want = p[t_off: t_off + rows * cols].view(rows, cols).t().contiguous().to(BF).view(-1)
    assert torch.equal(buf[pad: pad + rows * cols], want)
    assert bool(buf[:pad].isnan().all()) and bool(buf[pad + rows * cols:].isnan().all())
    assert torch.equal(shadow, p.to(BF))


def powf_probe(b, t0, n=8):
    """(device 1 - __powf(b, t), float64 1 - b^t) for t = t0 + 1, read off an update in which
    everything else is exact: b2 = 0 (v' = g^2, bc2 = 1), g = 1, eps = 0, lr = 1, p = 0, m = 0 give
    p' = -fl(fl(1 - b) / bc1): one correctly rounded division (U / 2 relative) of known numbers."""
    C = _lib()
    p, g = torch.zeros(n, device=DEV), torch.ones(n, device=DEV)
    m, v = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    step = torch.zeros(4, device=DEV)
    step[0] = float(t0)
    C.adam_dev(p, g, m, v, step, 1.0, b, 0.0, 0.0, 0.0, 1.0, None, False, None, 0, 0, 0, None, 0.0)
    torch.cuda.synchronize()
    b32 = R.f32(b)
    assert torch.equal(v.cpu(), torch.ones(n)) and torch.equal(m.cpu().double(), torch.full((n,), 1.0 - b32).double())
    assert bool((p == p[0]).all()) and p[0].item() < 0
    return (1.0 - b32) / -float(p[0].double().item()), 1.0 - b32 ** (t0 + 1)


def test_powf_error_is_within_delta():
    """The measured number: delta = |dev pow - b^t| / b^t with dev pow = 1 - (measured bc1), over
    b in {0.5, 0.9, 0.999} and every step number the tests above reach. The probe resolves bc1 to
    U / 2 relative, i.e. delta to (U / 2)(1 - x) / x with x = b^t: pairs with x >= 1/4 (1.5 U or
    better) bound DELTA_POWF = twice the worst of them (worst measured 1.68e-7, the probe's own
    rounding included); for every pair the term the tolerance really contains, delta x / (1 - x),
    is held against DELTA_POWF x / (1 - x) plus the probe's own 2 U."""
    worst, rows = 0.0, []
    for b in (0.5, 0.9, 0.999):
        for t0 in ADAM_T0:
            for k in range(STEPS):
                bc_dev, bc = powf_probe(b, t0 + k)
                x = 1.0 - bc
                rel_bc = abs(bc_dev - bc) / bc
                if x >= 0.25:
                    d = abs((1.0 - bc_dev) - x) / x
                    worst = max(worst, d)
                    rows.append((b, t0 + k + 1, d))
                assert rel_bc <= R.DELTA_POWF * x / bc + R.FLUSH / bc + 2 * R.U, (b, t0 + k + 1, bc_dev, bc)
    print("[powf] " + " ".join(f"b={b} t={t} delta={d:.3g}" for b, t, d in rows))
    print(f"[powf] worst delta {worst:.4g} (DELTA_POWF {R.DELTA_POWF:.4g})")
    assert worst <= R.DELTA_POWF


# ------------------------------------------------------------------------------ SGD
@pytest.mark.parametrize("n,hpname,nesterov", sgd_cases())
def test_sgd_dev_matches_fp64(n, hpname, nesterov):
    """sgd_dev_kernel: counter presets 0, 1 and 10^6, three steps; bit for bit on the lattice
    (decay 0), inside the derived bound otherwise. Worst measured error / bound: p 0.928, vel 0.931."""
    C, hp = _lib(), SGD_HP[hpname]
    ratios = {}
    p0, vel0, grads, cv = sgd_inputs(n, hpname)
    for it0, zero_g in zip(SGD_IT0, (True, False, True)):
        p, vel = p0.to(DEV), vel0.to(DEV)
        step = torch.zeros(4, device=DEV)
        step[0] = float(it0)
        clip = _clip_block(hp["clip"])
        for k, g_raw in enumerate(grads):
            before = (p.cpu(), vel.cpu())
            g = g_raw.to(DEV)
            C.sgd_dev(p, g, vel, step, hp["lr"], hp["decay"], hp["mu"], nesterov, hp["gscale"], zero_g, clip, cv)
            torch.cuda.synchronize()
            bad = sgd_violations((p.cpu(), vel.cpu()), before, g_raw, hp, cv, it0 + k, nesterov, ratios=ratios)
            assert not bad, f"sgd_dev n={n} {hpname} nesterov={nesterov} it={it0 + k}\n  " + "\n  ".join(bad)
            _counter(step, it0 + k + 1)
            assert torch.equal(g.cpu(), torch.zeros(n) if zero_g else g_raw), "bucket not cleared / not kept"
    _note("sgd_dev", ratios)


@pytest.mark.parametrize("n,hpname,nesterov", [c for c in sgd_cases() if c[1] in SGD_PLAIN_HP])
def test_sgd_host_lr_matches_fp64(n, hpname, nesterov):
    """sgd_kernel (lr_t from the host). Worst measured error / bound: p 0.779, vel 0.728."""
    C, hp = _lib(), SGD_HP[hpname]
    ratios = {}
    p0, vel0, grads, cv = sgd_inputs(n, hpname)
    lr, decay = R.f32(hp["lr"]), R.f32(hp["decay"])
    for it0 in SGD_IT0:
        p, vel = p0.to(DEV), vel0.to(DEV)
        for k, g_raw in enumerate(grads):
            before = (p.cpu(), vel.cpu())
            g = g_raw.to(DEV)
            C.sgd(p, g, vel, lr / (1.0 + decay * (it0 + k)), hp["mu"], nesterov, hp["gscale"])
            torch.cuda.synchronize()
            bad = sgd_violations((p.cpu(), vel.cpu()), before, g_raw, hp, cv, it0 + k, nesterov, host_lr=True,
                                 ratios=ratios)
            assert not bad, f"sgd n={n} {hpname} nesterov={nesterov} it={it0 + k}\n  " + "\n  ".join(bad)
            assert torch.equal(g.cpu(), g_raw)
    _note("sgd", ratios)


# ------------------------------------------------------------------------------ LSTM Adam + pack
LSTM_SHAPES = ((16, 128), (100, 128), (16, 256))  # KX 64, 128; H = 256: 320 tiles on 256 workgroups
LSTM_HP = tuple(ADAM_HP)
LSTM_T0 = (0, 999)


def _pack_encoders():
    """The host encoders of tests/test_lstm_pack_gpu.py (reused, not copied)."""
    import importlib.util
    import os

    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_lstm_pack_gpu.py")
    spec = importlib.util.spec_from_file_location("_lstm_pack_gpu_encoders", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod._weight_images


@pytest.mark.parametrize("F,H", LSTM_SHAPES)
def test_lstm_adam_pack_matches_fp64(F, H):
    """lstm_adam_pack_kernel through NativeLSTM + FlatAdam(writeback=eng): every parameter (the W
    block and the head) against adam_fp64, Wp / WhhT = the host encoders of the device's new
    parameters (from NaN prefill), the bucket cleared; every hyperparameter set at t = 1 and 1000.
    Worst measured error / bound: p 0.997, m 0.630, v 0.535."""
    from wellflow.models.lstm import NativeLSTM
    from wellflow.optim.flat import FlatAdam

    images = _pack_encoders()
    eng = NativeLSTM(F, H, 2, 32, device=DEV)
    n = eng.params.numel()
    KX = eng.lay.KX
    ratios = {}
    for hpname, t0 in itertools.product(LSTM_HP, LSTM_T0):
        hp = ADAM_HP[hpname]
        p0, m0, v0, grads, cv = adam_inputs(n, hpname, "nonzero" if t0 else "zero")
        opt = FlatAdam(eng.params, eng.grads, lr=ADAM_LR, betas=(hp["b1"], hp["b2"]), eps=hp["eps"],
                       weight_decay=hp["wd"], zero_grads=True, writeback=eng, clipvalue=cv)
        assert eng.fused_adam_ok(opt) and opt.clipnorm == 0.0
        opt.load_state_dict({**opt.state_dict(), "t": t0, "m": m0, "v": v0})
        if hp["clip"] is not None:  # the preset factor: FlatAdam hands the block over only with clipnorm on
            opt.clip_state[0] = hp["clip"]
            opt.clip_args = lambda gs, o=opt: (o.clip_state, o.clipvalue)
        eng.params.copy_(p0.to(DEV))
        eng.grads.copy_(grads[0].to(DEV))
        eng.Wp.fill_(NAN)
        eng.WhhT.fill_(NAN)
        opt.step(hp["gscale"])
        torch.cuda.synchronize()
        got = (eng.params.cpu(), opt.m.cpu(), opt.v.cpu())
        bad = adam_violations(got, (p0, m0, v0), grads[0], hp, cv, t0 + 1, ratios=ratios)
        assert not bad, f"lstm_adam_pack F={F} H={H} {hpname} t={t0 + 1}\n  " + "\n  ".join(bad)
        _counter(opt.step_dev, t0 + 1)
        assert eng.grads.abs().max().item() == 0.0, "bucket not cleared"
        Wp, WhhT = images(eng.lay.views(eng.params)[0], KX)
        assert torch.equal(eng.Wp, Wp) and torch.equal(eng.WhhT, WhhT)
    _note("lstm_adam_pack", ratios)
