"""The float64 optimizer references of wellflow/train/optim_ref.py and the input sets of the GPU
tests, without a GPU.

* the hand-written rules equal independent forms: float64 torch.optim.Adam / AdamW, the CPU
  branch of FlatAdam / FlatSGD (fp32, inside the fp32 bounds), a per-element Python loop;
* PLANTED ERRORS: for the exact input sets tests/test_optim_exact_gpu.py launches, each wrong
  rule of the list below, computed in float64 and rounded to fp32 (the best a kernel with that
  bug could do), is rejected by that file's own comparators at their own tolerances, on every
  step of every set the error can show on; the unmutated rule passes everywhere;
* the lattice sets really are exact in fp32, and every batch tests/test_small_exact_gpu.py
  launches satisfies the exactness conditions of wellflow/train/exact.py.
"""
import importlib.util
import itertools
import os

import pytest
import torch

from wellflow.optim.flat import FlatAdam, FlatSGD
from wellflow.train import optim_ref as R
from wellflow.train.cnn_exact import keras_sgd_fp64


def _load(name):
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), name + ".py")
    spec = importlib.util.spec_from_file_location("_cases_" + name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _load("test_optim_exact_gpu")
S = _load("test_small_exact_gpu")


def _rand(n, seed, scale=1.0):
    return scale * torch.randn(n, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


# ------------------------------------------------------------------------------ independent forms
@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("betas,eps", [((0.9, 0.999), 1e-8), ((0.5, 0.5), 1e-3)])
def test_adam_fp64_equals_torch_adam(betas, eps, wd):
    """Six steps with a new gradient each against float64 torch.optim.Adam (wd = 0) / AdamW."""
    n, lr = 257, 0.05
    p = torch.nn.Parameter(_rand(n, 1))
    cls = torch.optim.AdamW if wd else torch.optim.Adam
    opt = cls([p], lr=lr, betas=betas, eps=eps, weight_decay=wd)
    q, m, v = p.detach().clone(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    for t in range(1, 7):
        g = _rand(n, 10 + t)
        p.grad = g.clone()
        opt.step()
        q, m, v = R.adam_fp64(q, g, m, v, t, lr, betas[0], betas[1], eps, wd)
        assert torch.allclose(q, p.detach(), rtol=0, atol=1e-14), (t, (q - p.detach()).abs().max())
    st = opt.state[p]
    assert torch.allclose(m, st["exp_avg"], rtol=0, atol=1e-14) and torch.allclose(v, st["exp_avg_sq"], rtol=1e-13, atol=0)


def test_effective_gradient_forms_agree():
    g = _rand(1000, 3).float()
    for gs, fac, cv in [(1.0, None, 0.0), (1 / 64, 0.25, 0.01), (0.5, None, 0.3), (1 / 3, 0.7, 0.1)]:
        a = R.effective_grad_fp32(g, gs, fac, cv).double()
        b = R.effective_grad_fp64(g, R.f32(gs), 1.0 if fac is None else R.f32(fac), R.f32(cv))
        rel = R.grad_rel_error(gs, fac)
        assert bool(((a - b).abs() <= rel * b.abs() * R.SLACK).all())
        assert rel == 0.0 or not R.is_pow2(R.f32(gs) * (fac or 1.0))


@pytest.mark.parametrize("hpname", ["default", "wd_gs", "half_wd_cv"])
def test_flat_adam_cpu_branch_inside_fp32_bounds(hpname):
    """FlatAdam's CPU branch (fp32 torch operations in another order) over three steps: every
    step inside twice the kernel's own bounds of the float64 rule fed its state."""
    hp = G.ADAM_HP[hpname]
    n = 1025
    p0, m0, v0, grads, cv = G.adam_inputs(n, hpname, "nonzero")
    params, bucket = p0.clone(), torch.zeros(n)
    opt = FlatAdam(params, bucket, lr=G.ADAM_LR, betas=(hp["b1"], hp["b2"]), eps=hp["eps"], weight_decay=hp["wd"],
                   clipvalue=cv)
    opt.m.copy_(m0)
    opt.v.copy_(v0)
    # the CPU branch is handed Python floats: those, not their fp32 roundings, are its exact inputs
    b1, b2, eps, wd, lr = hp["b1"], hp["b2"], hp["eps"], hp["wd"], G.ADAM_LR
    for k, g in enumerate(grads):
        before = (params.clone(), opt.m.clone(), opt.v.clone())
        bucket.copy_(g)
        opt.step(hp["gscale"])
        pn, mn, vn = R.adam_fp64(*before[:1], g, *before[1:], k + 1, lr, b1, b2, eps, wd, hp["gscale"], 1.0, cv)
        ge = R.effective_grad_fp64(g, hp["gscale"], 1.0, cv)
        # torch rounds each scalar to fp32 where it meets the tensor (U each)
        tol_p = 2 * R.adam_p_tol(before[0], ge, before[1], mn, vn, pn, k + 1, lr, b1, b2, eps, wd, delta=0.0)
        tol_p = tol_p + 4 * R.U * (pn - before[0].double()).abs()
        assert bool(((opt.m.double() - mn).abs() <= 2 * R.adam_m_tol(ge, before[1], b1) + 2 * R.U * mn.abs()).all())
        assert bool(((opt.v.double() - vn).abs() <= 2 * R.adam_v_tol(vn) + 2 * R.U * vn.abs()).all())
        assert bool(((params.double() - pn).abs() <= tol_p).all()), ((params.double() - pn).abs() / tol_p).max()


@pytest.mark.parametrize("nesterov", [True, False])
@pytest.mark.parametrize("hpname", ["lattice", "decay"])
def test_flat_sgd_cpu_branch_inside_fp32_bounds(hpname, nesterov):
    hp = G.SGD_HP[hpname]
    n = 257
    p0, vel0, grads, cv = G.sgd_inputs(n, hpname)
    params, bucket = p0.clone(), torch.zeros(n)
    opt = FlatSGD(params, bucket, lr=hp["lr"], momentum=hp["mu"], decay=hp["decay"], nesterov=nesterov, clipvalue=cv)
    opt.vel.copy_(vel0)
    opt.iterations = 1000
    lr, mu, decay = hp["lr"], hp["mu"], hp["decay"]  # Python floats: the CPU branch's exact inputs
    for k, g in enumerate(grads):
        before = (params.clone(), opt.vel.clone())
        bucket.copy_(g)
        opt.step(hp["gscale"])
        pn, vn = R.sgd_fp64(before[0], g, before[1], 1000 + k, lr, mu, nesterov, decay, hp["gscale"], 1.0, cv)
        ge = R.effective_grad_fp64(g, hp["gscale"], 1.0, cv)
        e_p, e_v = R.sgd_tol(pn, ge, before[1], vn, 1000 + k, lr, mu, nesterov, decay)
        # torch rounds lr_t and momentum to fp32 where they meet the tensor: U each
        e_v = 2 * e_v + 4 * R.U * vn.abs()
        e_p = 2 * e_p + 8 * R.U * (pn - before[0].double()).abs()
        assert bool(((opt.vel.double() - vn).abs() <= e_v).all())
        assert bool(((params.double() - pn).abs() <= e_p).all())
    assert opt.iterations == 1003


@pytest.mark.parametrize("nesterov", [True, False])
def test_sgd_fp64_equals_a_python_loop(nesterov):
    n, lr, mu, decay, it = 50, 0.1, 0.9, 1e-6, 12345
    p, g, v = _rand(n, 1), _rand(n, 2), _rand(n, 3, 0.1)
    pn, vn = R.sgd_fp64(p, g, v, it, lr, mu, nesterov, decay, gscale=0.5, clip_factor=0.25, clipvalue=0.05)
    for i in range(n):
        ge = max(-0.05, min(0.05, float(g[i]) * 0.5 * 0.25))
        lr_t = lr / (1.0 + decay * it)
        vi = mu * float(v[i]) - lr_t * ge
        pi = float(p[i]) + (mu * vi - lr_t * ge if nesterov else vi)
        assert abs(vi - float(vn[i])) <= 1e-16 and abs(pi - float(pn[i])) <= 1e-15
    assert bool((g.abs() * 0.125 > 0.05).any()) and bool((g.abs() * 0.125 < 0.05).any())
    a, b = keras_sgd_fp64(p, g, v, lr, mu, nesterov, decay, it)
    c, d = R.sgd_fp64(p, g, v, it, lr, mu, nesterov, decay)
    assert torch.equal(a, c) and torch.equal(b, d)


def test_adam_moments_fp32_is_the_zero_state_step():
    g = _rand(4096, 5).float()
    for b1, b2 in ((0.9, 0.999), (0.5, 0.5)):
        m32, v32 = R.adam_moments_fp32(g, b1, b2)
        z = torch.zeros_like(g)
        _, mn, vn = R.adam_fp64(z, g, z, z, 1, 0.0, R.f32(b1), R.f32(b2), 1e-8)
        assert bool(((m32.double() - mn).abs() <= R.adam_m_tol(g, z, R.f32(b1))).all())
        assert bool(((v32.double() - vn).abs() <= R.adam_v_tol(vn)).all())


# ------------------------------------------------------------------------------ planted errors
def _ge(g, gscale, fac, cv, mode):
    g = g.double()
    if mode == "clamp_before_scale":
        return (g.clamp(-cv, cv) if cv > 0 else g) * gscale * fac
    if mode == "clip_ignored":
        fac = 1.0
    if mode == "gscale_twice":
        gscale = gscale * gscale
    return R.effective_grad_fp64(g, gscale, fac, cv)


def adam_mutant(mode, p, g, m, v, t, lr, b1, b2, eps, wd, gscale, fac, cv):
    """adam_fp64 with one planted error (``mode`` None: the rule itself, written a second time)."""
    p, m, v = p.double(), m.double(), v.double()
    ge = _ge(g, gscale, fac, cv, mode)
    if mode == "b2_099":
        b2 = 0.99
    if mode == "wd_coupled":
        ge = ge + wd * p
    mn = b1 * m + (1 - b1) * ge
    vn = b2 * v + (1 - b2) * ge * ge
    tb = t - 1 if mode == "t_minus_1" else (t + 1 if mode == "t_plus_1" else t)
    mh, vh = mn / (1 - b1 ** tb), vn / (1 - b2 ** tb)
    den = (vh + eps).sqrt() if mode == "eps_in_sqrt" else vh.sqrt() + eps
    decay = 0.0 if mode in ("wd_coupled", "wd_dropped") else wd
    return p - lr * (mh / den + decay * p), mn, vn


ADAM_MUTANTS = ("b2_099", "t_minus_1", "t_plus_1", "eps_in_sqrt", "wd_coupled", "wd_dropped", "clamp_before_scale",
                "clip_ignored", "gscale_twice")


def adam_mutant_shows(mode, hp, cv, t):
    """Whether the planted error changes anything on this set (else it cannot be rejected there)."""
    if mode in ("t_minus_1", "t_plus_1"):  # both corrections are 1 to fp32 once b^t is gone
        return max(hp["b1"] ** t, hp["b2"] ** t) >= 1e-3
    if mode in ("wd_coupled", "wd_dropped"):
        return hp["wd"] != 0.0
    if mode == "clamp_before_scale":
        return cv > 0 and G._scale_of(hp) != 1.0
    if mode == "clip_ignored":
        return hp["clip"] is not None
    if mode == "gscale_twice":
        return hp["gscale"] != 1.0
    return True


def _adam_args(hp, cv):
    return dict(lr=R.f32(G.ADAM_LR), b1=R.f32(hp["b1"]), b2=R.f32(hp["b2"]), eps=R.f32(hp["eps"]), wd=R.f32(hp["wd"]),
                gscale=R.f32(hp["gscale"]), fac=1.0 if hp["clip"] is None else hp["clip"], cv=cv)


def _adam_sets(sizes, t0s, starts=("zero", "nonzero")):
    for (n, hpname), t0, start in itertools.product([c for c in G.adam_cases() if c[0] in sizes], t0s, starts):
        yield n, hpname, t0, start


def _walk_adam(n, hpname, t0, start):
    """(before, g, t, float64 step rounded to fp32) along the three steps of a set, the state
    carried in fp32 as the device carries it."""
    hp = G.ADAM_HP[hpname]
    p, m, v, grads, cv = G.adam_inputs(n, hpname, start)
    for k, g in enumerate(grads):
        t = t0 + k + 1
        nxt = tuple(x.float() for x in adam_mutant(None, p, g, m, v, t, **_adam_args(hp, cv)))
        if not bool(m.any()) and not bool(v.any()):  # from zero state fp32 has ONE answer (not float64's, rounded)
            nxt = (nxt[0],) + R.adam_moments_fp32(R.effective_grad_fp32(g, hp["gscale"], hp["clip"], cv), hp["b1"], hp["b2"])
        yield (p, m, v), g, t, nxt, hp, cv
        p, m, v = nxt


@pytest.mark.parametrize("sizes,t0s,starts", [((1023, 1025), G.ADAM_T0, ("zero", "nonzero")),
                                              ((262149,), (0, 999), ("nonzero",))])
def test_adam_comparator_rejects_every_planted_error(sizes, t0s, starts):
    shown = {m: 0 for m in ADAM_MUTANTS}
    for n, hpname, t0, start in _adam_sets(sizes, t0s, starts):
        for before, g, t, nxt, hp, cv in _walk_adam(n, hpname, t0, start):
            tag = f"n={n} {hpname} t={t} start={start}"
            assert not G.adam_violations(nxt, before, g, hp, cv, t), f"the rule itself is rejected: {tag}"
            for mode in ADAM_MUTANTS:
                if not adam_mutant_shows(mode, hp, cv, t):
                    continue
                got = tuple(x.float() for x in adam_mutant(mode, *before[:1], g, *before[1:], t, **_adam_args(hp, cv)))
                assert G.adam_violations(got, before, g, hp, cv, t), f"planted error {mode} passes: {tag}"
                shown[mode] += 1
    assert all(shown.values()), shown


def test_adam_reference_written_twice_agrees():
    for before, g, t, nxt, hp, cv in _walk_adam(1025, "wd_gs_clip", 9, "nonzero"):
        a = adam_mutant(None, *before[:1], g, *before[1:], t, **_adam_args(hp, cv))
        k = _adam_args(hp, cv)
        b = R.adam_fp64(before[0], g, before[1], before[2], t, k["lr"], k["b1"], k["b2"], k["eps"], k["wd"], k["gscale"],
                        k["fac"], k["cv"])
        for x, y in zip(a, b):
            assert torch.allclose(x, y, rtol=1e-15, atol=1e-300)


def sgd_mutant(mode, p, g, vel, it, lr, mu, nesterov, decay, gscale, fac, cv):
    ge = _ge(g, gscale, fac, cv, mode)
    if mode == "nesterov_flipped":
        nesterov = not nesterov
    lr_t = lr / (1 + decay * (it + 1 if mode == "lr_t_next" else it))
    vn = mu * vel.double() - lr_t * ge
    return p.double() + (mu * vn - lr_t * ge if nesterov else vn), vn


SGD_MUTANTS = ("nesterov_flipped", "lr_t_next", "clamp_before_scale", "clip_ignored", "gscale_twice")


def sgd_mutant_shows(mode, hp, cv):
    if mode == "lr_t_next":
        return hp["decay"] != 0.0
    if mode == "clamp_before_scale":
        return cv > 0 and G._scale_of(hp) != 1.0
    if mode == "clip_ignored":
        return hp["clip"] is not None
    if mode == "gscale_twice":
        return hp["gscale"] != 1.0
    return True


@pytest.mark.parametrize("sizes", [(255, 257), (524289,)])
def test_sgd_comparator_rejects_every_planted_error(sizes):
    shown = {m: 0 for m in SGD_MUTANTS}
    for (n, hpname, nesterov), it0 in itertools.product([c for c in G.sgd_cases() if c[0] in sizes], G.SGD_IT0):
        hp = G.SGD_HP[hpname]
        p, vel, grads, cv = G.sgd_inputs(n, hpname)
        args = dict(lr=R.f32(hp["lr"]), mu=R.f32(hp["mu"]), nesterov=nesterov, decay=R.f32(hp["decay"]),
                    gscale=R.f32(hp["gscale"]), fac=1.0 if hp["clip"] is None else hp["clip"], cv=cv)
        for k, g in enumerate(grads):
            it = it0 + k
            tag = f"n={n} {hpname} nesterov={nesterov} it={it}"
            nxt = tuple(x.float() for x in sgd_mutant(None, p, g, vel, it, **args))
            for host_lr in (False, True):
                if host_lr and hpname not in G.SGD_PLAIN_HP:
                    continue
                assert not G.sgd_violations(nxt, (p, vel), g, hp, cv, it, nesterov, host_lr), f"rule rejected: {tag}"
                for mode in SGD_MUTANTS:
                    if not sgd_mutant_shows(mode, hp, cv):
                        continue
                    got = tuple(x.float() for x in sgd_mutant(mode, p, g, vel, it, **args))
                    assert G.sgd_violations(got, (p, vel), g, hp, cv, it, nesterov, host_lr), \
                        f"planted error {mode} passes: {tag} host_lr={host_lr}"
                    shown[mode] += 1
            p, vel = nxt
    assert all(shown.values()), shown


# ------------------------------------------------------------------------------ the lattices
def test_adam_lattice_sets_are_exact_in_fp32():
    """b = 0.5 on dyadic moments and gradients: m' and v' of every step are fp32 numbers (so
    'bit for bit' is the only right answer), whichever way the multiply-adds are fused."""
    lattice = [h for h in G.ADAM_HP if G.ADAM_HP[h]["lattice"]]
    assert lattice and all(G.ADAM_HP[h]["b1"] == 0.5 == G.ADAM_HP[h]["b2"] for h in lattice)
    for n, hpname, t0, start in _adam_sets((5, 1025), (0,)):
        if hpname not in lattice:
            continue
        for before, g, t, nxt, hp, cv in _walk_adam(n, hpname, t0, start):
            _, mn, vn = adam_mutant(None, *before[:1], g, *before[1:], t, **_adam_args(hp, cv))
            ge = R.effective_grad_fp64(g, R.f32(hp["gscale"]), 1.0 if hp["clip"] is None else hp["clip"], cv)
            for x in (mn, vn, 0.5 * ge, 0.5 * ge * ge, 0.5 * before[1].double(), 0.5 * before[2].double()):
                assert torch.equal(x.float().double(), x)
            if cv > 0:
                assert bool((ge.abs() == cv).any()) and bool((ge.abs() < cv).any())


def test_sgd_lattice_sets_are_exact_in_fp32():
    for (n, hpname, nesterov), it0 in itertools.product([c for c in G.sgd_cases() if c[0] == 257], G.SGD_IT0):
        hp = G.SGD_HP[hpname]
        if not hp["lattice"]:
            continue
        assert hp["decay"] == 0.0
        p, vel, grads, cv = G.sgd_inputs(n, hpname)
        fac = 1.0 if hp["clip"] is None else hp["clip"]
        for k, g in enumerate(grads):
            ge = R.effective_grad_fp64(g, hp["gscale"], fac, cv)
            assert set(ge.tolist()) <= ({-2.0, -1.0, 0.0, 1.0, 2.0} if cv == 0 else {-1.0, -0.5, 0.0, 0.5, 1.0})
            if cv > 0:  # the clamp bites on some elements, others lie inside it
                raw = g.double() * hp["gscale"] * fac
                assert bool((raw.abs() > cv).any()) and bool((raw.abs() < cv).any()) and bool((raw.abs() == cv).any())
            pn, vn = R.sgd_fp64(p, g, vel, it0 + k, hp["lr"], hp["mu"], nesterov, 0.0, hp["gscale"], fac, cv)
            for x in (pn, vn, hp["mu"] * vel.double(), hp["lr"] * ge, hp["mu"] * vn):
                assert torch.equal(x.float().double(), x)
            p, vel = pn.float(), vn.float()


def test_input_sets_can_tell_the_rules_apart():
    """Clamps bite on some elements and not on others; dead elements exist; tiny ones too."""
    for hpname, hp in G.ADAM_HP.items():
        p0, m0, v0, grads, cv = G.adam_inputs(1025, hpname, "nonzero")
        ge = R.effective_grad_fp32(grads[0], hp["gscale"], hp["clip"], 0.0)
        assert bool(((ge == 0) & (m0 == 0) & (v0 == 0)).any()) and bool(m0.any()) and bool(v0.any())
        if hp["cv"]:
            assert bool((ge.abs() == cv).any()) and bool((ge.abs() > cv).any()) and bool((ge.abs() < cv).any())
        else:
            assert cv == 0.0
    for n in G.ADAM_N:  # the smallest sizes still carry a live element
        assert bool(G.adam_inputs(n, "default", "zero")[3][0].any())


# ------------------------------------------------------------------------------ the small-batch MLP batches
@pytest.mark.parametrize("key", S.one_step_keys() + S.k_step_keys(), ids=lambda k: "-".join(map(str, k)))
def test_small_batches_are_exact(key):
    bt = S.batches(*key)
    assert not bt.violations(), bt.tag
    lay = bt.lay
    for ref in bt.refs:
        gl, ghw, ghb = lay.views(ref["grads"])
        for name, blk in (("dW1", gl[0][0]), ("db1", gl[0][1]), ("dW2", gl[1][0]), ("db2", gl[1][1]), ("dw3", ghw)):
            assert float(blk.abs().max()) > 0, f"{bt.tag}: {name} is all zero"
        assert bool((gl[0][0][:, bt.F:] == 0).all())  # W1's padding columns carry no gradient
        assert torch.equal(ref["grads"].float().double(), ref["grads"])
    total = S.LOSS_ACC0
    for ref in bt.refs:  # the loss accumulator after every step is an fp32 number
        total = total + ref["loss_sum"]
        assert torch.equal(total.float().double(), total)
    if bt.steps > 1:
        assert len({tuple(bt.rows[k * bt.B: (k + 1) * bt.B].tolist()) for k in range(bt.steps)}) == bt.steps
        assert not torch.equal(bt.refs[0]["grads"], bt.refs[1]["grads"])
        # m after K steps with betas 0.5, from zero and from the previous launch's moments: on the fp32 lattice
        z = torch.zeros(lay.numel)
        m, v, _ = S.k_step_moments(bt, z, z)
        assert torch.equal(m.float().double(), m)
        m2, _, _ = S.k_step_moments(bt, m.float(), v.float())
        assert torch.equal(m2.float().double(), m2)
        mk = torch.zeros(lay.numel, dtype=torch.float64)
        for ref in bt.refs:  # and every intermediate m with its two terms, whichever way it is fused
            for x in (0.5 * ref["grads"], 0.5 * mk, 0.5 * mk + 0.5 * ref["grads"]):
                assert torch.equal(x.float().double(), x)
            mk = 0.5 * mk + 0.5 * ref["grads"]
