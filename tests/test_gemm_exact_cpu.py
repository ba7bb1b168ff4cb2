"""The exact GEMM cases of wellflow/train/gemm_exact.py, proved without a GPU.

* every case tests/test_gemm_exact_gpu.py launches meets the exactness conditions, and holds the
  values it is listed for (ties and both rounding directions in ``outH``, zero and negative ReLU
  pre-activations, all five mask values, ...);
* ``gemm_fp64`` equals a per-element triple loop;
* the comparator the GPU file uses rejects each of a list of planted kernel errors, applied to
  the float64 result of a case that exercises it;
* the route of every case, from the launcher's own plan function (no launch, CPU tensors), is the
  one the table lists it for, and the table covers every route the router can produce.
"""
import dataclasses

import numpy as np
import pytest
import torch

from wellflow.train import gemm_exact as gx
from wellflow.train.gemm_exact import CASE_BY_NAME, CASES


def _ids(c):
    return c.name


# ------------------------------------------------------------------------------ the conditions
@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_every_case_is_exact(case):
    assert gx.gemm_exactness_violations(case) == []


def test_table_scope():
    """The extents, option values and special cases the table must hold."""
    assert 60 <= len(CASES) <= 110
    assert {c.M for c in CASES} >= {1, 8, 37, 120, 128, 136, 264}
    assert {c.N for c in CASES} >= {8, 12, 120, 128, 132, 136}
    assert {c.K for c in CASES} >= {8, 56, 64, 72, 128, 192, 256, 448, 1000}
    assert all(c.K <= 1024 for c in CASES)
    assert {c.K // 64 for c in CASES if c.mainloop == "ring"} >= {1, 2, 3, 4, 7}
    assert {c.alpha for c in CASES} == {1.0, 0.5} and {c.beta for c in CASES} == {0.0, 0.25, -1.0}
    assert {c.mask_scale for c in CASES} == {1.0, 2.0} and {c.drop_p for c in CASES} == {0.0, 0.5}
    assert {c.out for c in CASES} == {"F", "H", "FH"}
    for c in CASES:
        assert not (c.a_mn and c.M % 8) and not (c.b_mn and c.N % 8), c.name
    by = lambda **kw: [c for c in CASES if all(getattr(c, k) == v for k, v in kw.items())]  # noqa: E731
    for ep in ("staged", "direct"):
        assert [c for c in by(epilogue=ep, colsum=True) if c.M % 128], ep
        assert [c for c in by(epilogue=ep, mask=True) if c.ldm_pad] and [c for c in by(epilogue=ep, mask=True) if not c.ldm_pad]
        assert [c for c in by(epilogue=ep, out="H")], ep
    assert [c for c in by(drop_p=0.5, epilogue="direct", out="F", step=None)]
    assert [c for c in by(drop_p=0.5, epilogue="direct", out="F") if c.step and c.ldo_pad]
    assert [c for c in by(epilogue="staged") if c.ldo_pad % 8 == 0 and c.ldo_pad]
    assert [c for c in by(epilogue="direct", out="H") if c.ldo_pad % 8]
    assert [c for c in CASES if c.lda_pad and c.ldb_pad and not c.a_mn and not c.b_mn]
    assert [c for c in CASES if c.lda_pad and c.ldb_pad and c.a_mn and c.b_mn]
    assert [c for c in by(atomic=True) if c.alpha == 0.5 and c.K == 200 and c.ksplit == 3]
    assert by(kernel="dw256x128", tile=1)[0].N % 128


def test_operands_are_asymmetric_and_dense():
    c = CASE_BY_NAME["KxK-ring1-128x128x64"]
    d = gx.gemm_data(c)
    ref = gx.gemm_fp64(c, d)["v"]
    assert not torch.equal(ref, ref.t())
    for c in CASES:
        d = gx.gemm_data(c)
        assert bool((d.B != 0).all()), c.name
        if c.M == c.K:
            assert not torch.equal(d.A, d.A.t()), c.name


def test_mask_lattice_holds_the_smallest_normal_and_both_zeros():
    d = gx.gemm_data(CASE_BY_NAME["mask-staged"])
    stored = d.mask.to(torch.bfloat16)
    assert torch.equal(stored.double(), d.mask)                       # 2^-126 is a bf16 number
    assert bool((stored.double() == 2.0 ** -126).any())
    signs = np.signbit(d.mask.numpy())
    assert bool(((d.mask == 0) & torch.from_numpy(signs)).any()) and bool(((d.mask == 0) & ~torch.from_numpy(signs)).any())


# --------------------------------------------------------------------------- the reference
def _loop_reference(case, d):
    """gemm_fp64, one element at a time, in Python floats."""
    M, N, K = case.M, case.N, case.K
    A, B = d.A.tolist(), d.B.tolist()
    v = torch.zeros(M, N, dtype=torch.float64)
    for m in range(M):
        for n in range(N):
            acc = 0.0
            for k in range(K):
                acc += A[m][k] * B[n][k]
            x = case.alpha * acc
            if case.atomic:
                v[m, n] = x + float(d.prior[m, n])
                continue
            if case.beta != 0.0:
                x += case.beta * float(d.prior[m, n])
            if d.bias is not None:
                x += float(d.bias[n])
            if case.act == 1:
                x = max(x, 0.0)
            if d.keep is not None:
                x = x * 2.0 if bool(d.keep[m, n]) else 0.0
            if d.mask is not None:
                x = x * case.mask_scale if float(d.mask[m, n]) > 0 else 0.0
            v[m, n] = x
    return v


@pytest.mark.parametrize("name", ["mask-direct-F", "dropout-direct-F", "beta-0.25", "atomic-KxK-ks2", "colsum-direct-F"])
def test_reference_equals_triple_loop(name):
    case = CASE_BY_NAME[name]
    d = gx.gemm_data(case)
    ref = gx.gemm_fp64(case, d)
    v = _loop_reference(case, d)
    assert torch.equal(ref["v"], v)
    if ref["colsum"] is not None:
        assert torch.equal(ref["colsum"], d.csum0 + v.sum(0))


def test_census_counts_by_hand():
    v = torch.tensor([257.0, 514.0, 1028.0, 256.0, 258.0, 129.25, 129.75, -129.25, -129.75, 0.0, 3.5])
    c = gx.rounding_census(v.double())
    assert c == {"exact": 4, "tie": 3, "up": 2, "down": 2}
    assert gx.to_bf16_fp64(torch.tensor([257.0, 259.0], dtype=torch.float64)).tolist() == [256.0, 260.0]  # to even


# ----------------------------------------------------------------------------- planted errors
def _as_got(case, res):
    """A result dict as the host buffers the GPU test reads back: the window inside NaN."""
    got = {}
    R = case.M + gx.OUT_SPARE_ROWS
    for name, dt in (("outF", torch.float32), ("outH", torch.bfloat16)):
        if res.get(name) is not None:
            got[name] = torch.full((R, case.ldo), float("nan"), dtype=dt)
            got[name][: case.M, : case.N] = res[name].to(dt)
    if res.get("colsum") is not None:
        got["colsum"] = torch.cat([res["colsum"].float(), torch.full((5,), float("nan"))])
    return got


def _epilogue(case, d, acc, *, bias_shift=0, bias_after_relu=False, drop_beta=False, alpha_on_bias=False, mask_rule="gt",
              ignore_mask_scale=False, keep=None, truncate=False):
    """The epilogue written out once more, with switches for the errors a kernel could make."""
    v = case.alpha * acc
    if case.atomic:
        v = v + d.prior
        return {"v": v, "outF": v, "outH": None, "colsum": None}
    bias = None if d.bias is None else torch.roll(d.bias, -bias_shift)
    if case.beta != 0.0 and not drop_beta:
        v = v + case.beta * d.prior
    if bias is not None and not bias_after_relu:
        v = v + (case.alpha * bias if alpha_on_bias else bias)
    if case.act == 1:
        v = v.clamp(min=0.0)
    if bias is not None and bias_after_relu:
        v = v + bias
    keep = d.keep if keep is None else keep
    if keep is not None:
        v = torch.where(keep, 2.0 * v, torch.zeros_like(v))
    if d.mask is not None:
        on = {"gt": d.mask > 0, "ge": d.mask >= 0, "ne": d.mask != 0}[mask_rule]
        v = torch.where(on, v * (1.0 if ignore_mask_scale else case.mask_scale), torch.zeros_like(v))
    if truncate:
        vb = (v.float().view(torch.int32) & -65536).view(torch.float32).double()
    else:
        vb = gx.to_bf16_fp64(v)
    cs = None if d.csum0 is None else d.csum0 + (vb if case.epilogue == "staged" else v).sum(0)
    return {"v": v, "outF": v if "F" in case.out else None, "outH": vb if "H" in case.out else None, "colsum": cs}


def _rejected(case, wrong, ref):
    bad = gx.gemm_mismatches(case, _as_got(case, wrong), ref)
    assert bad, f"{case.name}: the planted error was not noticed"
    return {line.split(":")[0]: line for line in bad}


def _setup(name):
    case = CASE_BY_NAME[name]
    d = gx.gemm_data(case)
    ref = gx.gemm_fp64(case, d)
    acc = d.A @ d.B.t()
    right = _epilogue(case, d, acc)
    assert gx.gemm_mismatches(case, _as_got(case, right), ref) == []  # the rewritten epilogue, unswitched, is the reference
    return case, d, ref, acc


def _count(line):
    return int(line.split(":")[1].split()[0])


def test_planted_transposed_c():
    case, d, ref, acc = _setup("KxK-ring1-128x128x64")
    assert case.M == case.N
    wrong = dict(ref, outF=ref["outF"].t().contiguous())
    assert "outF" in _rejected(case, wrong, ref)


@pytest.mark.parametrize("name,k0,k1", [("KxK-ring-direct-264x120x256", 64, 128), ("atomic-192-ks2", 128, 192),
                                         ("MNxMN-register-direct-128x136x1000", 960, 1000)])
def test_planted_dropped_k_step(name, k0, k1):
    """One 64-deep k-step of a four-step problem; the last (64-deep) k-step of the short second
    split; the zero-filled 40-deep tail of K = 1000."""
    case, d, ref, acc = _setup(name)
    A = d.A.clone()
    A[:, k0:k1] = 0.0
    v = case.alpha * (A @ d.B.t()) + (d.prior if case.atomic else 0.0)
    if d.bias is not None:
        v = v + d.bias
    bad = _rejected(case, dict(ref, outF=v), ref)
    assert _count(bad["outF"]) > 0.9 * case.M * case.N  # nearly every element moves


def test_planted_bias_errors():
    case, d, ref, acc = _setup("bias-direct")
    assert "outF" in _rejected(case, _epilogue(case, d, acc, bias_shift=1), ref)
    case, d, ref, acc = _setup("bias-relu-direct")
    bad = _rejected(case, _epilogue(case, d, acc, bias_after_relu=True), ref)
    pre = case.alpha * acc
    assert _count(bad["outF"]) == int((((pre + d.bias).clamp(min=0)) != (pre.clamp(min=0) + d.bias)).sum())
    case, d, ref, acc = _setup("alpha-0.5-F")
    bad = _rejected(case, _epilogue(case, d, acc, alpha_on_bias=True), ref)
    assert _count(bad["outF"]) == case.M * int((d.bias != 0).sum())


def test_planted_beta_dropped():
    case, d, ref, acc = _setup("beta-0.25")
    bad = _rejected(case, _epilogue(case, d, acc, drop_beta=True), ref)
    assert _count(bad["outF"]) == int((d.prior != 0).sum())


def test_planted_mask_rules():
    case, d, ref, acc = _setup("mask-staged")
    unmasked = gx.to_bf16_fp64(case.alpha * acc)
    bad = _rejected(case, _epilogue(case, d, acc, mask_rule="ge"), ref)
    assert _count(bad["outH"]) == int(((d.mask == 0) & (unmasked != 0)).sum())     # the +-0.0 entries, nothing else
    bad = _rejected(case, _epilogue(case, d, acc, mask_rule="ne"), ref)
    assert _count(bad["outH"]) == int(((d.mask < 0) & (unmasked != 0)).sum())
    case, d, ref, acc = _setup("mask-direct-F")
    bad = _rejected(case, _epilogue(case, d, acc, ignore_mask_scale=True), ref)
    assert _count(bad["outF"]) == int(((d.mask > 0) & (acc != 0)).sum())


def test_planted_dropout_key_uses_ldo():
    from wellflow.train.cnn_exact import uniform_hash

    case, d, ref, acc = _setup("dropout-direct-F-step")
    assert case.ldo > case.N and case.step is not None
    s = (gx.DROP_SEED ^ ((case.step * 0xD1B54A32D192ED03) & ((1 << 64) - 1)))
    idx = (np.arange(case.M, dtype=np.uint64)[:, None] * np.uint64(case.ldo) + np.arange(case.N, dtype=np.uint64)[None, :])
    keep = torch.from_numpy(uniform_hash(s, idx.reshape(-1)) >= np.float32(0.5)).reshape(case.M, case.N)
    assert torch.equal(keep[0], d.keep[0]) and not torch.equal(keep[1:], d.keep[1:])  # row 0 has the same keys
    bad = _rejected(case, _epilogue(case, d, acc, keep=keep), ref)
    assert "first at (m, n) = (1," in bad["outF"]


def test_planted_truncation_into_outH():
    case, d, ref, acc = _setup("KxK-register-staged-136x120x72")
    c = gx.rounding_census(ref["v"])
    bad = _rejected(case, _epilogue(case, d, acc, truncate=True), ref)
    assert c["up"] <= _count(bad["outH"]) <= c["up"] + c["tie"]


def test_planted_colsum_errors():
    # a row m >= M of the over-read tile summed as well
    case, d, ref, acc = _setup("colsum-direct-F-ring")
    ghost = case.alpha * (torch.full((case.K,), 0.5, dtype=torch.float64) @ d.B.t())
    assert bool((ghost != 0).any())
    bad = _rejected(case, dict(ref, colsum=ref["colsum"] + ghost), ref)
    assert _count(bad["colsum"]) == int((ghost != 0).sum()) and "outF" not in bad
    # the other epilogue's rule
    for name in ("colsum-direct-H-N132", "colsum-staged"):
        case, d, ref, acc = _setup(name)
        other = dataclasses.replace(case, epilogue="staged" if case.epilogue == "direct" else "direct")
        bad = _rejected(case, gx.gemm_fp64(other, d), ref)
        assert list(bad) == ["colsum"]


def test_window_guard_notices_a_write_outside():
    case, d, ref, acc = _setup("F-ldo-pad")
    got = _as_got(case, ref)
    got["outF"][0, case.N] = 0.0           # the first column of the gap
    assert gx.gemm_mismatches(case, got, ref)[0].startswith("outF outside")
    got = _as_got(case, ref)
    got["outF"][case.M, 0] = 1.0           # the first row past M
    assert gx.gemm_mismatches(case, got, ref)[0].startswith("outF outside")


# --------------------------------------------------------------------------------- the routes
def _plan(case):
    from wellflow.ops.native import gemm_plan

    buf = gx.gemm_buffers(case, gx.gemm_data(case))
    sd = torch.tensor([case.step], dtype=torch.int64) if case.step is not None else None
    return gemm_plan(buf["A"], buf["B"], case.M, case.N, case.K, **gx.gemm_kwargs(case, buf, sd))


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_case_takes_the_route_it_is_listed_for(case):
    """From the launcher's own decision function, without a launch."""
    p = _plan(case)
    assert (p["kernel"], p["mainloop"], p["epilogue"]) == (case.kernel, case.mainloop, case.epilogue), p


def test_table_covers_every_route():
    cov = gx.route_coverage()
    assert set(cov) == gx.REQUIRED_ROUTES, set(cov) ^ gx.REQUIRED_ROUTES
    assert {k: v for k, v in cov.items() if v != {"M", "N", "K"}} == {}
    assert any(c.kernel == "dw256x128" and c.N % 128 for c in CASES)


def test_plan_numbers():
    """kchunk / nsplit / workgroups of the split-K and multi-tile cases."""
    want = {"atomic-192-ks2": (128, 2, 4), "atomic-200-ks3": (128, 2, 4), "atomic-128-ks8": (64, 2, 4),
            "atomic-grid18": (64, 3, 18), "atomic-grid12": (64, 2, 12), "atomic-tile1-256x136": (64, 2, 4),
            "grid6-264x136x256-H": (256, 1, 6)}
    for name, (kchunk, nsplit, wgs) in want.items():
        p = _plan(CASE_BY_NAME[name])
        assert (p["kchunk"], p["nsplit"], p["workgroups"]) == (kchunk, nsplit, wgs), (name, p)
    assert any(w >= 9 and w % 8 for _, _, w in want.values())
