"""gemm_kernel (csrc/gemm.hip) against float64, BIT FOR BIT, on every route and epilogue option.

The data (wellflow/train/gemm_exact.py) is chosen so that nothing but ``f2bf`` into ``outH`` ever
rounds: whatever order the MFMAs, the split-K atomics and the colsum atomics add in, the kernel
must reproduce the float64 reference exactly. There is no tolerance in this file. The case table
lives in the host module; tests/test_gemm_exact_cpu.py proves every case exact without a GPU and
shows that the comparator used here rejects a list of planted kernel errors.

Every output buffer is larger than the M x N window and prefilled with NaN; after the launch
everything outside the window (columns N .. ldo - 1, rows >= M, colsum[N:]) must still be NaN.
Operands of ring cases are allocated up to the next 128-row boundary and the spare region (like
every gap of lda / ldb) holds NaN: the ring reads it, every product that touches it belongs to
a discarded row or column, so the result must still be exact and NaN-free.

The route of each case (kernel, mainloop, epilogue) is asserted from ``gemm_plan``, the function
the launcher itself decides with, and the set of routes the table reaches is compared with the
set the router can produce.

Pinned behaviours (csrc/gemm.hip header, ops/native.py gemm): colsum sums the bf16-rounded values
on the staged epilogue and the unrounded ones on the direct epilogue; atomic refuses bias / mask /
colsum / act / drop_p; act outside {0, 1} and drop_p outside [0, 1) are refused.
"""
import dataclasses
import functools

import pytest
import torch

from wellflow.train import gemm_exact as gx
from wellflow.train.gemm_exact import CASE_BY_NAME, CASES

pytestmark = pytest.mark.gpu
DEV = "cuda"


@functools.lru_cache(maxsize=None)
def problem(name):
    """(case, data, float64 reference): computed once, shared, never modified."""
    case = CASE_BY_NAME[name]
    d = gx.gemm_data(case)
    return case, d, gx.gemm_fp64(case, d)


def launch(case, d, step="case"):
    """Run the case on the device; returns (the plan, the host copies of what it wrote into)."""
    from wellflow.ops.native import gemm, gemm_plan

    buf = {k: v.to(DEV) for k, v in gx.gemm_buffers(case, d).items()}
    step = case.step if step == "case" else step
    sd = torch.tensor([step], dtype=torch.int64, device=DEV) if step is not None else None
    kw = gx.gemm_kwargs(case, buf, sd)
    plan = gemm_plan(buf["A"], buf["B"], case.M, case.N, case.K, **kw)
    gemm(buf["A"], buf["B"], case.M, case.N, case.K, **kw)
    torch.cuda.synchronize()
    return plan, {k: buf[k].cpu() for k in ("outF", "outH", "colsum") if k in buf}


@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_gemm_case_matches_fp64(name):
    case, d, ref = problem(name)
    bad = gx.gemm_exactness_violations(case, d)
    assert not bad, f"{name}: the case is not exact, nothing launched: {bad}"
    plan, got = launch(case, d)
    assert (plan["kernel"], plan["mainloop"], plan["epilogue"]) == (case.kernel, case.mainloop, case.epilogue), plan
    bad = gx.gemm_mismatches(case, got, ref)
    assert not bad, f"{name} {plan}:\n  " + "\n  ".join(bad)
    for k in ("outF", "outH"):                                  # bit for bit, stated once more without the helper
        if ref[k] is not None:
            assert (got[k][: case.M, : case.N].double() != ref[k]).nonzero().shape[0] == 0


def test_routes_reached_are_the_routes_the_router_has():
    """A set comparison, from the plans of the device tensors: every (layout, mainloop, epilogue)
    of the generic kernel, each with an M tail, an N tail and a K edge; the 256x128 tile with an
    N tail; grids of 6, 12 (not a multiple of 8) and 18 workgroups."""
    from wellflow.ops.native import gemm_plan

    plans = {}
    for case in CASES:
        buf = {k: v.to(DEV) for k, v in gx.gemm_buffers(case, problem(case.name)[1]).items()}
        sd = torch.zeros(1, dtype=torch.int64, device=DEV) if case.step is not None else None
        plans[case.name] = gemm_plan(buf["A"], buf["B"], case.M, case.N, case.K, **gx.gemm_kwargs(case, buf, sd))
    routed = [dataclasses.replace(c, kernel=plans[c.name]["kernel"], mainloop=plans[c.name]["mainloop"],
                                     epilogue=plans[c.name]["epilogue"]) for c in CASES]
    cov = gx.route_coverage(routed)
    assert set(cov) == gx.REQUIRED_ROUTES, set(cov) ^ gx.REQUIRED_ROUTES
    assert {k: v for k, v in cov.items() if v != {"M", "N", "K"}} == {}
    assert [c for c in routed if c.kernel == "dw256x128" and c.tile == 1 and c.N % 128]
    grids = {p["workgroups"] for p in plans.values()}
    assert {6, 12, 18} <= grids
    assert plans["atomic-200-ks3"]["nsplit"] == 2 and plans["atomic-128-ks8"]["nsplit"] == 2


def test_another_step_counter_is_rejected():
    """Negative control on the device: the same launch reading step counter + 1 draws another
    dropout mask, and the comparator reports it (so the comparisons above do look at what the
    kernel wrote)."""
    case, d, ref = problem("dropout-direct-F-step")
    _, got = launch(case, d, step=case.step + 1)
    bad = gx.gemm_mismatches(case, got, ref)
    assert [line.split(":")[0] for line in bad] == ["outF"], bad
    _, got = launch(case, d, step=None)         # and no counter at all is a third stream
    assert [line.split(":")[0] for line in gx.gemm_mismatches(case, got, ref)] == ["outF"]


# ------------------------------------------------------------------------ wellflow::linear_act
def _linear_problem(M, K, N, act):
    from wellflow.train.exact import _pick, _sum_ok

    g = torch.Generator().manual_seed(1000 * M + 10 * K + N + act)
    x = _pick(gx.A_VALUES, (M, K), g)
    W = _pick(gx.B_VALUES, (N, K), g)
    b = _pick(gx.BIAS_VALUES, (N,), g)
    dy = _pick((-1.0, -0.5, -0.25, 0.0, 0.25, 0.5, 1.0), (M, N), g)
    z = x @ W.t() + b
    y = z.clamp(min=0.0) if act else z
    dz = dy * (y > 0).double() if act else dy
    ref = {"y": gx.to_bf16_fp64(y), "dx": dz @ W, "dW": dz.t() @ x, "db": dz.sum(0)}
    bad = []
    _sum_ok("z", x.abs() @ W.abs().t() + b.abs(), 0.25, bad)
    _sum_ok("dx", dz.abs() @ W.abs(), 0.125, bad)
    _sum_ok("dW", dz.abs().t() @ x.abs(), 0.125, bad)
    _sum_ok("db", dz.abs().sum(0), 0.25, bad)
    assert not bad and torch.equal(dz.to(torch.bfloat16).double(), dz), bad
    if act:
        assert bool((z == 0).any()) and bool((z < 0).any())
    return x, W, b, dy, ref


@pytest.mark.parametrize("act", (0, 1))
@pytest.mark.parametrize("M,K,N", [(40, 13, 12), (136, 64, 128), (257, 40, 96)])
def test_linear_act_matches_fp64(M, K, N, act):
    """y (bf16), dx, dW and db of the custom op on lattice data, bit for bit: the zero padding of
    K and N to multiples of 8, the K x K -> outH forward (direct at N = 12), the direct K x MN ->
    outF route of dX that nothing else uses, and the split-K MN x MN dW over K = M rows."""
    import wellflow.ops.torch_ops  # noqa: F401  (registers wellflow::*)
    from wellflow.ops.native import gemm_plan
    from wellflow.train.cnn_exact import block_mismatches

    x64, W64, b64, dy64, ref = _linear_problem(M, K, N, act)
    x = x64.float().to(DEV).requires_grad_(True)
    W = W64.float().to(DEV).requires_grad_(True)
    b = b64.float().to(DEV).requires_grad_(True)
    y = torch.ops.wellflow.linear_act(x, W, b, act)
    y.backward(dy64.to(torch.bfloat16).to(DEV))
    torch.cuda.synchronize()
    got = {"y": y.detach().cpu(), "dx": x.grad.cpu(), "dW": W.grad.cpu(), "db": b.grad.cpu()}
    want = {"y": ref["y"].to(torch.bfloat16), "dx": ref["dx"].float(), "dW": ref["dW"].float(), "db": ref["db"].float()}
    bad = block_mismatches(got, want)
    assert not bad, f"linear_act M={M} K={K} N={N} act={act}:\n  " + "\n  ".join(bad)
    # the dX call of ops/torch_ops.py (A = dZ [M][Np], B = W as an MN-contiguous [Np][Kp] image)
    Np, Kp = (N + 7) // 8 * 8, (K + 7) // 8 * 8
    p = gemm_plan(torch.zeros(M, Np, dtype=torch.bfloat16), torch.zeros(Np, Kp, dtype=torch.bfloat16), M, Kp, Np,
                  b_mn=True, ldb=Kp, outF=torch.zeros(M, Kp))
    assert (p["kernel"], p["epilogue"]) == ("generic", "direct")


# ------------------------------------------------------------------------------------ refusals
ATOMIC_EXTRAS = {"bias": lambda N: dict(bias=torch.zeros(N, device=DEV)),
                 "mask": lambda N: dict(mask=torch.ones(128, N, device=DEV, dtype=torch.bfloat16)),
                 "colsum": lambda N: dict(colsum=torch.zeros(N, device=DEV)),
                 "act": lambda N: dict(act=1),
                 "drop_p": lambda N: dict(drop_p=0.5)}


def _refused(match, **kw):
    """The call must raise on the host with ``match`` and leave the output as it was."""
    from wellflow.ops.native import gemm, gemm_plan

    M = N = K = 128
    A = torch.ones(M, K, device=DEV, dtype=torch.bfloat16)
    B = torch.ones(N, K, device=DEV, dtype=torch.bfloat16)
    out = torch.full((M, N), float("nan"), device=DEV)
    for fn in (gemm, gemm_plan):
        with pytest.raises(RuntimeError, match=match):
            fn(A, B, M, N, K, outF=out, **kw)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    for v in kw.values():
        if isinstance(v, torch.Tensor) and v.dtype == torch.float32:
            assert float(v.abs().max()) == 0.0   # colsum / bias untouched as well


@pytest.mark.parametrize("extra", sorted(ATOMIC_EXTRAS))
def test_atomic_refuses_what_it_would_ignore(extra):
    _refused(r"atomic adds alpha \* acc only; bias, mask, colsum, act and drop_p cannot go with it",
             atomic=True, **ATOMIC_EXTRAS[extra](128))


@pytest.mark.parametrize("act", (-1, 2, 3))
def test_unknown_act_is_refused(act):
    _refused(rf"act must be 0 \(linear\) or 1 \(ReLU\), got {act}", act=act)


@pytest.mark.parametrize("p", (1.0, 1.5, -0.25, float("nan")))
def test_drop_p_outside_unit_interval_is_refused(p):
    _refused(r"drop_p must lie in \[0, 1\), got", drop_p=p)


def test_mask_scale_without_a_mask_is_fine():
    from wellflow.ops.native import gemm

    case, d, ref = problem("KxK-ring1-128x128x64")
    buf = {k: v.to(DEV) for k, v in gx.gemm_buffers(case, d).items()}
    kw = gx.gemm_kwargs(case, buf)
    kw["mask_scale"] = 2.0
    gemm(buf["A"], buf["B"], case.M, case.N, case.K, **kw)
    torch.cuda.synchronize()
    assert gx.gemm_mismatches(case, {"outF": buf["outF"].cpu()}, ref) == []
