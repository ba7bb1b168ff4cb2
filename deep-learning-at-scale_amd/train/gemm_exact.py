"""The general MFMA GEMM on data where bf16 / fp32 arithmetic is exact (tests/test_gemm_exact_*.py).

The recipe of train/exact.py and train/cnn_exact.py for ``gemm_kernel`` (csrc/gemm.hip): operands,
bias, the prior output and every scale factor are small dyadic numbers, so that

* both operands survive the bf16 round trip;
* every fp32 accumulation (the MFMA k-loop in any order, the split-K atomics, the colsum
  atomics) is a sum of multiples of one quantum, far below 2^24 quanta;
* alpha, beta, mask_scale and the dropout keep scale are powers of two (or -1).

The ONLY rounding of the whole operation is then ``f2bf`` into ``outH``, and a plain float64
computation (:func:`gemm_fp64`) must be matched BIT FOR BIT by every route of the kernel: four
operand layouts, the register-staged and the direct-to-LDS ring mainloop, the staged and the direct
epilogue. :func:`gemm_exactness_violations` proves the conditions for one case, so a mismatch on
the device can only be the kernel or a host predicate.

The lattice: A in {-2 .. 2, step 0.5}, B in {+-0.5, +-1} (dense: every fragment slot holds a value
a misplaced slot would change; both operands random, so neither is symmetric or an identity),
bias in {0, +-0.5, +-1, +-1.5}, alpha in {1, 0.5}, beta in {0, 0.25, -1} with the prior ``outF``
in {-2 .. 2, step 0.5}, mask_scale in {1, 2}, drop_p in {0, 0.5} (keep scale 2), mask entries in
{+1, -1, +0.0, -0.0, 2^-126} (the smallest positive normal must count as ``> 0``). No subnormals.

Cases that write ``outH`` must also exercise its rounding: on this lattice |v| < 64 is always a
bf16 number, so six rows of A and six rows of B are made "heavy" (A mostly 2, B mostly 1: outputs
near alpha * 1.85 K), which puts exact ties between two bf16 neighbours and values that round up
and down among the outputs. K >= 72 is needed for that; such cases carry no ``outH`` below it.

The rule for ``colsum`` follows the route (csrc/gemm.hip header): the staged epilogue sums the
bf16-rounded values it stores, the direct one the unrounded fp32 values.

Order of operations, as in the kernel: ``alpha * acc``, ``+ beta * out``, ``+ bias``, ReLU, dropout
(key ``m * N + n``), mask (``> 0`` keeps, times ``mask_scale``).
"""
from __future__ import annotations

import dataclasses

import numpy as np
import torch

from .cnn_exact import block_mismatches, gemm_dropout_mask
from .exact import MAX_QUANTA, _pick, _roundtrip_ok, _sum_ok, quantum

A_VALUES = (-2.0, -1.5, -1.0, -0.5, 0.0, 0.5, 1.0, 1.5, 2.0)
B_VALUES = (-1.0, -0.5, 0.5, 1.0)
BIAS_VALUES = (-1.5, -1.0, -0.5, 0.0, 0.5, 1.0, 1.5)
PRIOR_VALUES = A_VALUES
CSUM_VALUES = (-3.0, -1.5, 0.5, 2.0)            # what colsum holds before the launch: never zero
MASK_VALUES = (1.0, -1.0, 0.0, -0.0, 2.0 ** -126)
HEAVY = 6                                       # heavy rows of A and of B in a case that writes outH
HEAVY_MIN_K = 72
DROP_SEED = 0x5EED5                             # host seed of every dropout case
NAN = float("nan")


@dataclasses.dataclass(frozen=True)
class GemmCase:
    name: str
    M: int
    N: int
    K: int
    a_mn: bool = False
    b_mn: bool = False
    spare: bool = False        # operands allocated up to the next 128 rows (NaN there): the ring may run
    lda_pad: int = 0           # leading dimensions beyond the tight ones (gaps hold NaN)
    ldb_pad: int = 0
    out: str = "F"             # "F", "H" or "FH"
    ldo_pad: int = 0
    bias: bool = False
    act: int = 0
    alpha: float = 1.0
    beta: float = 0.0
    mask: bool = False
    ldm_pad: int = 0           # ldm = ldo + ldm_pad
    mask_scale: float = 1.0
    colsum: bool = False
    drop_p: float = 0.0
    step: int | None = None    # the device step counter (seed_dev) the launch reads; None = no counter
    atomic: bool = False
    ksplit: int = 1
    tile: int = 0
    seed: int = 0
    kernel: str = "generic"    # the route the case is in the table for (asserted from gemm_plan)
    mainloop: str = "register"
    epilogue: str = "direct"

    @property
    def lda(self) -> int:
        return (self.M if self.a_mn else self.K) + self.lda_pad

    @property
    def ldb(self) -> int:
        return (self.N if self.b_mn else self.K) + self.ldb_pad

    @property
    def ldo(self) -> int:
        return self.N + self.ldo_pad

    @property
    def ldm(self) -> int:
        return self.ldo + self.ldm_pad

    @property
    def layout(self) -> str:
        return ("MN" if self.a_mn else "K") + "x" + ("MN" if self.b_mn else "K")

    @property
    def heavy(self) -> bool:
        return "H" in self.out


@dataclasses.dataclass
class GemmData:
    """One case's values (float64, logical shapes). ``prior`` is what ``outF`` holds before the
    launch (the beta term and the atomic target; zeros when neither reads it)."""
    A: torch.Tensor            # [M][K]
    B: torch.Tensor            # [N][K]
    bias: torch.Tensor | None  # [N]
    prior: torch.Tensor        # [M][N]
    mask: torch.Tensor | None  # [M][N]
    csum0: torch.Tensor | None  # [N]
    keep: torch.Tensor | None  # [M][N] bool: the dropout keep mask


def gemm_data(case: GemmCase) -> GemmData:
    """The case's values on the lattice (module docstring), drawn from ``case.seed``."""
    g = torch.Generator(device="cpu").manual_seed(case.seed)
    M, N, K = case.M, case.N, case.K
    A = _pick(A_VALUES, (M, K), g)
    B = _pick(B_VALUES, (N, K), g)
    if case.heavy:
        if K < HEAVY_MIN_K:
            raise ValueError(f"{case.name}: a case that writes outH needs K >= {HEAVY_MIN_K}")
        ra = torch.randperm(M, generator=g)[:HEAVY]
        rb = torch.randperm(N, generator=g)[:HEAVY]
        A[ra] = torch.where(torch.rand(len(ra), K, generator=g) < 0.9, 2.0, 1.5).double()
        B[rb] = torch.where(torch.rand(len(rb), K, generator=g) < 0.9, 1.0, 0.5).double()
    bias = _pick(BIAS_VALUES, (N,), g) if case.bias else None
    reads_prior = case.beta != 0.0 or case.atomic
    prior = _pick(PRIOR_VALUES, (M, N), g) if reads_prior else torch.zeros(M, N, dtype=torch.float64)
    mask = _pick(MASK_VALUES, (M, N), g) if case.mask else None
    csum0 = _pick(CSUM_VALUES, (N,), g) if case.colsum else None
    keep = gemm_dropout_mask(DROP_SEED, case.step, M, N, case.drop_p) if case.drop_p > 0 else None
    return GemmData(A, B, bias, prior, mask, csum0, keep)


def to_bf16_fp64(v: torch.Tensor) -> torch.Tensor:
    """float64 values through ``.float().to(torch.bfloat16)`` (round to nearest even), as float64."""
    return v.float().to(torch.bfloat16).double()


def gemm_pre_fp64(case: GemmCase, d: GemmData) -> torch.Tensor:
    """alpha * A B^T + beta * prior + bias in float64: the value ReLU sees ([M][N])."""
    v = case.alpha * (d.A @ d.B.t())
    if case.atomic:
        return v + d.prior
    if case.beta != 0.0:
        v = v + case.beta * d.prior
    if d.bias is not None:
        v = v + d.bias
    return v


def gemm_fp64(case: GemmCase, d: GemmData | None = None) -> dict:
    """The launch in plain float64: ``v`` (the unrounded result [M][N]), ``outF`` (= v), ``outH``
    (v rounded to bf16, as float64) and ``colsum`` (the prefilled vector plus the column sums of
    what the case's epilogue has in hand: the rounded values when ``case.epilogue`` is "staged",
    the unrounded ones when "direct"); None for what the case does not write."""
    d = gemm_data(case) if d is None else d
    v = gemm_pre_fp64(case, d)
    if not case.atomic:
        if case.act == 1:
            v = torch.where(v > 0, v, torch.zeros_like(v))
        if d.keep is not None:
            v = torch.where(d.keep, v * (1.0 / (1.0 - case.drop_p)), torch.zeros_like(v))
        if d.mask is not None:
            v = torch.where(d.mask > 0, v * case.mask_scale, torch.zeros_like(v))
    vb = to_bf16_fp64(v)
    colsum = None
    if d.csum0 is not None:
        colsum = d.csum0 + (vb if case.epilogue == "staged" else v).sum(0)
    return {"v": v, "outF": v if "F" in case.out else None, "outH": vb if "H" in case.out else None, "colsum": colsum}


def rounding_census(v: torch.Tensor) -> dict:
    """How the values of ``v`` (float64, fp32 numbers) round to bf16: ``exact``, ``tie`` (half way
    between two bf16 neighbours), ``up`` / ``down`` (not a tie; rounded away from / towards zero:
    truncation gets every ``up`` and half the ties wrong)."""
    f = v.float().reshape(-1)
    assert torch.equal(f.double(), v.reshape(-1)), "not fp32 numbers"
    bits = f.view(torch.int32)
    lo = (bits & -65536).view(torch.float32).double().abs()           # truncated towards zero
    hi = ((bits & -65536) + 65536).view(torch.float32).double().abs()   # the next bf16 away from zero
    a = v.reshape(-1).abs()
    exact = a == lo
    tie = ~exact & ((a - lo) == (hi - a))
    rb = to_bf16_fp64(v).reshape(-1).abs()
    up = ~exact & ~tie & (rb == hi)
    down = ~exact & ~tie & (rb == lo)
    return {"exact": int(exact.sum()), "tie": int(tie.sum()), "up": int(up.sum()), "down": int(down.sum())}


def gemm_exactness_violations(case: GemmCase, d: GemmData | None = None) -> list:
    """Why a kernel could legitimately differ from :func:`gemm_fp64` on this case, or why the case
    would not test what it is listed for; an empty list when

    (a) A, B and the mask survive the bf16 round trip and hold no subnormal; bias, the prior
        output, the prefilled colsum and the results survive the fp32 round trip;
    (b) per output element, sum |a||b|, then with |beta * prior| and |bias| added, stays below
        2^24 quanta of its terms, so the MFMA order and the split-K atomic order cannot matter, and
        alpha, the keep scale and mask_scale are powers of two;
    (c) the colsum's sum of |terms| (the prefill included) stays below 2^24 quanta;
    (d) a case that writes outH holds at least one exact tie, one value rounded up and one rounded
        down among the values it rounds; a ReLU case holds a pre-activation that is exactly 0 and
        a negative one; a mask case holds all five mask values inside the window; a dropout case
        drops and keeps; a colsum case on rounding data gives different sums under the two rules."""
    d = gemm_data(case) if d is None else d
    bad: list = []
    bf, f32 = torch.bfloat16, torch.float32
    _roundtrip_ok("A", d.A, bf, bad)
    _roundtrip_ok("B", d.B, bf, bad)
    tiny = 2.0 ** -126
    for name, t in (("A", d.A), ("B", d.B), ("bias", d.bias), ("prior", d.prior), ("mask", d.mask)):
        if t is not None and bool(((t != 0) & (t.abs() < tiny)).any()):
            bad.append(f"{name}: holds a subnormal")
    for s in (case.alpha, case.mask_scale, 1.0 / (1.0 - case.drop_p)):
        if quantum(torch.tensor([s])) != abs(s):
            bad.append(f"scale {s} is no power of two")
    ref = gemm_fp64(case, d)
    v = ref["v"]
    _roundtrip_ok("result", v, f32, bad)
    _roundtrip_ok("prior outF", d.prior, f32, bad)
    ab = d.A.abs() @ d.B.abs().t()
    qab = quantum(d.A) * quantum(d.B)
    _sum_ok("sum |a||b|", ab, qab, bad)
    terms, q = abs(case.alpha) * ab, abs(case.alpha) * qab
    if case.beta != 0.0 or case.atomic:
        beta = 1.0 if case.atomic else case.beta
        terms, q = terms + abs(beta) * d.prior.abs(), min(q, abs(beta) * quantum(d.prior))
        _sum_ok("alpha * acc + beta * prior", terms, q, bad)
    if d.bias is not None:
        _roundtrip_ok("bias", d.bias, f32, bad)
        terms, q = terms + d.bias.abs(), min(q, quantum(d.bias))
        _sum_ok("... + bias", terms, q, bad)
    scale = (1.0 / (1.0 - case.drop_p)) * case.mask_scale
    _sum_ok("the scaled result", scale * terms, q, bad)
    if d.mask is not None:
        _roundtrip_ok("mask", d.mask, bf, bad)
        # +0.0 and -0.0 are told apart by their sign bit
        seen = {(float(x), bool(np.signbit(float(x)))) for x in d.mask.reshape(-1).tolist()}
        if len(seen) != len(MASK_VALUES):
            bad.append(f"mask: only {len(seen)} of the {len(MASK_VALUES)} mask values appear")
    if d.csum0 is not None:
        _roundtrip_ok("colsum prefill", d.csum0, f32, bad)
        _roundtrip_ok("colsum", ref["colsum"], f32, bad)
        summed = to_bf16_fp64(v) if case.epilogue == "staged" else v
        _sum_ok("colsum", d.csum0.abs() + summed.abs().sum(0), min(quantum(summed), quantum(d.csum0)), bad)
        if bool((d.csum0 == 0).any()):
            bad.append("colsum prefill holds a zero")
    if case.heavy:
        c = rounding_census(v)
        if min(c["tie"], c["up"], c["down"]) < 1:
            bad.append(f"outH: the values rounded hold {c}: a tie, a value rounded up and one rounded down are needed")
        if d.csum0 is not None and torch.equal(v.sum(0), to_bf16_fp64(v).sum(0)):
            bad.append("colsum: the rounded and the unrounded column sums are the same numbers")
    if case.act == 1:
        pre = gemm_pre_fp64(case, d)
        if not (bool((pre == 0).any()) and bool((pre < 0).any())):
            bad.append("ReLU: no pre-activation that is exactly 0, or none that is negative")
    if d.keep is not None and (bool(d.keep.all()) or not bool(d.keep.any())):
        bad.append("dropout: the mask keeps everything or nothing")
    return bad


# ------------------------------------------------------------------------------- device buffers
def _rows128(n: int) -> int:
    return (n + 127) // 128 * 128


def operand_image(x: torch.Tensor, mn: bool, ld: int, spare: bool) -> torch.Tensor:
    """The bf16 storage of a logical [rows][K] operand: K-contiguous [rows][ld] or MN-contiguous
    [K][ld]; gaps (columns beyond the tight extent) hold NaN. ``spare``: the allocation also holds
    what a whole 128-row tile may over-read (rows up to the next multiple of 128 for K-contiguous,
    enough further k-rows for MN-contiguous), all NaN; else it ends with the last row."""
    rows, K = x.shape
    Rc = _rows128(rows)
    if mn:
        nk = K + ((Rc - rows + ld - 1) // ld if spare else 0)
        buf = torch.full((nk, ld), NAN, dtype=torch.float64)
        buf[:K, :rows] = x.t()
    else:
        buf = torch.full((Rc if spare else rows, ld), NAN, dtype=torch.float64)
        buf[:rows, :K] = x
    return buf.to(torch.bfloat16)


OUT_SPARE_ROWS = 3  # rows past M of every output buffer: never written


def gemm_buffers(case: GemmCase, d: GemmData) -> dict:
    """Host tensors of everything the launch is given, each larger than the M x N window it may
    touch: ``A`` / ``B`` (:func:`operand_image`), ``outF`` (the prior values inside the window when
    the launch reads them, NaN everywhere else), ``outH`` (NaN), ``mask`` ([rows][ldm], 1 outside
    the window), ``bias`` (N, then NaN), ``colsum`` (the prefill, then NaN)."""
    M, N = case.M, case.N
    R = M + OUT_SPARE_ROWS
    buf = {"A": operand_image(d.A, case.a_mn, case.lda, case.spare),
           "B": operand_image(d.B, case.b_mn, case.ldb, case.spare)}
    if "F" in case.out:
        o = torch.full((R, case.ldo), NAN, dtype=torch.float32)
        if case.beta != 0.0 or case.atomic:
            o[:M, :N] = d.prior.float()
        buf["outF"] = o
    if "H" in case.out:
        buf["outH"] = torch.full((R, case.ldo), NAN, dtype=torch.bfloat16)
    if d.mask is not None:
        m = torch.ones(R, case.ldm, dtype=torch.float64)
        m[:M, :N] = d.mask
        buf["mask"] = m.to(torch.bfloat16)
    if d.bias is not None:
        buf["bias"] = torch.cat([d.bias.float(), torch.full((5,), NAN)])
    if d.csum0 is not None:
        buf["colsum"] = torch.cat([d.csum0.float(), torch.full((5,), NAN)])
    return buf


def gemm_kwargs(case: GemmCase, buf: dict, seed_dev=None) -> dict:
    """The keyword arguments of ops.native.gemm / gemm_plan for the case over ``buf`` (on any device)."""
    kw = dict(a_mn=case.a_mn, lda=case.lda, b_mn=case.b_mn, ldb=case.ldb, outF=buf.get("outF"), outH=buf.get("outH"),
              ldo=case.ldo, bias=buf.get("bias"), mask=buf.get("mask"), ldm=case.ldm, mask_scale=case.mask_scale,
              colsum=buf.get("colsum"), alpha=case.alpha, beta=case.beta, act=case.act, atomic=case.atomic,
              ksplit=case.ksplit, drop_p=case.drop_p, seed=DROP_SEED if case.drop_p > 0 else 0, tile=case.tile)
    if seed_dev is not None:
        kw["seed_dev"] = seed_dev
    return kw


# ---------------------------------------------------------------------------------- comparator
def gemm_mismatches(case: GemmCase, got: dict, ref: dict) -> list:
    """:func:`cnn_exact.block_mismatches` over what the case writes: per output buffer (host
    tensors, as :func:`gemm_buffers` shaped them) the M x N window against the float64 reference
    cast to the buffer's type, with the first differing (m, n) added, and ``<name> outside``: every
    element outside the window must still be NaN. ``colsum``: the first N entries against the
    reference, the rest still NaN."""
    M, N = case.M, case.N
    g, w = {}, {}
    for name, dt in (("outF", torch.float32), ("outH", torch.bfloat16)):
        if ref.get(name) is None:
            continue
        full = got[name]
        g[name], w[name] = full[:M, :N].contiguous(), ref[name].to(dt)
        outside = torch.isnan(full)
        outside[:M, :N] = True
        g[name + " outside"], w[name + " outside"] = outside, torch.ones_like(outside)
    if ref.get("colsum") is not None:
        g["colsum"], w["colsum"] = got["colsum"][:N].contiguous(), ref["colsum"].float()
        g["colsum outside"] = torch.isnan(got["colsum"][N:])
        w["colsum outside"] = torch.ones_like(g["colsum outside"])
    bad = block_mismatches(g, w)
    for i, line in enumerate(bad):
        name = line.split(":")[0]
        if name in ("outF", "outH") and g[name].shape == w[name].shape:
            m, n = (g[name] != w[name]).nonzero()[0].tolist()
            bad[i] = f"{line}; first at (m, n) = ({m}, {n})"
    return bad


# ---------------------------------------------------------------------------------- case table
LAYOUTS = ((False, False), (False, True), (True, False), (True, True))
RING_SHAPES = ((120, 136, 128), (264, 120, 256), (136, 128, 448))   # 2 / 4 / 7 k-steps, M and N tails
REG_SHAPES = ((120, 136, 128), (136, 120, 72), (128, 136, 1000))    # tight tails; zero-filled k tails


def _table() -> tuple:
    cases = []

    def add(name, M, N, K, **kw):
        kw.setdefault("seed", 100 + len(cases))
        cases.append(GemmCase(name=name, M=M, N=N, K=K, **kw))

    # every (layout, mainloop, epilogue) the router can produce for tile 0, each with an M tail, an
    # N tail and a K edge (ring: a k-step count that is no multiple of its 3 stages; register:
    # K % 64 != 0), and (120, 136, 128) through both mainloops
    for a_mn, b_mn in LAYOUTS:
        lay = ("MN" if a_mn else "K") + "x" + ("MN" if b_mn else "K")
        for ep in ("staged", "direct"):
            opts = dict(out="H", bias=True) if ep == "staged" else dict(out="F")
            for i, (M, N, K) in enumerate(RING_SHAPES):
                add(f"{lay}-ring-{ep}-{M}x{N}x{K}", M, N, K, a_mn=a_mn, b_mn=b_mn, spare=True, mainloop="ring",
                    epilogue=ep, act=1 if (ep == "staged" and i == 1) else 0, **opts)
            for i, (M, N, K) in enumerate(REG_SHAPES):
                add(f"{lay}-register-{ep}-{M}x{N}x{K}", M, N, K, a_mn=a_mn, b_mn=b_mn, epilogue=ep,
                    bias=(ep == "staged" or i == 2), **{k: v for k, v in opts.items() if k != "bias"})
        # small and single-step problems (outF: below K = 72 nothing rounds): the smallest extents a
        # layout admits, ring laps of 1 and 3 k-steps (whole tiles need no spare allocation)
        Ms, Ns = (8 if a_mn else 1), (8 if b_mn else 12)
        add(f"{lay}-tiny-{Ms}x{Ns}x8", Ms, Ns, 8, a_mn=a_mn, b_mn=b_mn, bias=True)
        add(f"{lay}-small-{8 if a_mn else 37}x{Ns}x56", 8 if a_mn else 37, Ns, 56, a_mn=a_mn, b_mn=b_mn)
        add(f"{lay}-ring1-128x128x64", 128, 128, 64, a_mn=a_mn, b_mn=b_mn, mainloop="ring", bias=True, act=1)
        add(f"{lay}-ring3-8x8x192", 8, 8, 192, a_mn=a_mn, b_mn=b_mn, spare=True, mainloop="ring")

    # multi-tile grids: 6 tiles; with split-K 3, 18 workgroups; 12 workgroups (not a multiple of 8)
    add("grid6-264x136x256-H", 264, 136, 256, spare=True, mainloop="ring", epilogue="staged", out="H", bias=True, act=1)
    add("grid6-264x136x72-F", 264, 136, 72, b_mn=True, bias=True)

    # split-K atomics on the generic kernel (tile 0): a nonzero prior outF, alpha 0.5
    at = dict(a_mn=True, b_mn=True, atomic=True, alpha=0.5)
    add("atomic-192-ks2", 136, 120, 192, ksplit=2, spare=True, mainloop="ring", **at)       # kchunk 128, then 64
    add("atomic-200-ks3", 136, 120, 200, ksplit=3, **at)                                     # 128, then 72: register
    add("atomic-128-ks8", 120, 136, 128, ksplit=8, **at)                                     # more splits than k-steps
    add("atomic-grid18", 264, 136, 192, ksplit=3, spare=True, mainloop="ring", **at)        # 6 tiles x 3 splits
    add("atomic-grid12", 264, 136, 128, ksplit=2, **at)                                      # 12 workgroups, r = 4
    add("atomic-KxK-ks2", 37, 12, 192, ksplit=2, atomic=True, alpha=0.5)
    add("atomic-KxMN-ks2", 120, 136, 128, ksplit=2, b_mn=True, spare=True, mainloop="ring", atomic=True)
    add("atomic-MNxK-ks3", 136, 12, 200, ksplit=3, a_mn=True, atomic=True, alpha=0.5)
    # the 256x128 weight-gradient tile with an N tail (its generic epilogue masks the last column tile)
    add("atomic-tile1-256x136", 256, 136, 128, ksplit=2, tile=1, spare=True, kernel="dw256x128", mainloop="ring", **at)

    # epilogue options, on both epilogues where the route allows
    st = dict(out="H", epilogue="staged")
    add("bias-direct", 37, 12, 56, bias=True)
    add("bias-relu-direct", 37, 12, 56, bias=True, act=1)
    add("bias-relu-staged", 120, 136, 72, bias=True, act=1, **st)
    add("beta-0.25", 37, 12, 56, beta=0.25, bias=True)
    add("beta--1", 136, 120, 72, beta=-1.0, a_mn=True)
    add("beta-0.25-FH", 120, 136, 128, beta=0.25, out="FH", spare=True, mainloop="ring")
    add("alpha-0.5-F", 120, 136, 72, alpha=0.5, bias=True, b_mn=True)
    add("alpha-0.5-staged", 136, 120, 256, alpha=0.5, bias=True, a_mn=True, spare=True, mainloop="ring", **st)
    add("FH-together", 120, 136, 72, out="FH", bias=True, act=1)
    add("FH-together-MNxMN", 136, 120, 128, out="FH", a_mn=True, b_mn=True)
    add("H-direct-N12", 37, 12, 72, out="H", bias=True)
    add("H-direct-N132", 120, 132, 128, out="H", bias=True, act=1, a_mn=True, spare=True, mainloop="ring")
    add("H-direct-ldo-odd", 120, 136, 72, out="H", ldo_pad=4)
    add("H-staged-ldo-pad", 120, 136, 72, ldo_pad=8, bias=True, **st)
    add("F-ldo-pad", 37, 12, 56, ldo_pad=5, bias=True)
    add("mask-staged", 120, 136, 72, mask=True, b_mn=True, **st)
    add("mask-staged-ldm-pad", 136, 120, 128, mask=True, ldm_pad=16, mask_scale=2.0, b_mn=True, spare=True,
        mainloop="ring", **st)
    add("mask-direct-F", 37, 12, 56, mask=True, mask_scale=2.0)
    add("mask-direct-ldm-pad", 120, 136, 128, mask=True, ldm_pad=3, out="H", b_mn=True)
    add("mask-direct-FH", 136, 120, 128, mask=True, ldm_pad=8, out="FH", a_mn=True, b_mn=True)
    add("colsum-staged", 120, 136, 72, colsum=True, bias=True, act=1, **st)
    add("colsum-staged-mask", 264, 120, 128, colsum=True, mask=True, b_mn=True, spare=True, mainloop="ring", **st)
    add("colsum-direct-H-N132", 120, 132, 72, colsum=True, out="H", bias=True)
    add("colsum-direct-F", 37, 12, 56, colsum=True, bias=True, act=1)
    add("colsum-direct-F-ring", 264, 136, 128, colsum=True, mask=True, b_mn=True, spare=True, mainloop="ring")
    add("dropout-direct-F", 37, 12, 56, drop_p=0.5, bias=True, act=1)
    add("dropout-direct-F-step", 120, 136, 72, drop_p=0.5, step=7, ldo_pad=8, bias=True)
    add("dropout-direct-H-step", 120, 132, 72, drop_p=0.5, step=7, out="H", ldo_pad=3)
    add("dropout-staged-step", 136, 120, 128, drop_p=0.5, step=7, ldo_pad=8, bias=True, act=1, spare=True,
        mainloop="ring", **st)
    add("lda-ldb-pad-KxK", 120, 136, 72, lda_pad=8, ldb_pad=16, bias=True)
    add("lda-ldb-pad-KxK-ring", 120, 136, 128, lda_pad=16, ldb_pad=8, spare=True, mainloop="ring", **st)
    add("lda-ldb-pad-MNxMN", 120, 136, 72, a_mn=True, b_mn=True, lda_pad=8, ldb_pad=16)
    add("lda-ldb-pad-MNxMN-ring", 120, 136, 192, a_mn=True, b_mn=True, lda_pad=8, ldb_pad=120, spare=True,
        mainloop="ring", **st)
    names = [c.name for c in cases]
    assert len(set(names)) == len(names)
    return tuple(cases)


CASES = _table()
CASE_BY_NAME = {c.name: c for c in CASES}


def route_coverage(cases=CASES) -> dict:
    """{(layout, mainloop, epilogue): the set of edges ("M", "N", "K") its tile-0, non-atomic or
    atomic, generic-kernel cases show}: an M tail, an N tail (no multiple of 128) and a K edge (ring:
    a k-step count that is no multiple of 3; register: K % 64 != 0)."""
    cov: dict = {}
    for c in cases:
        if c.kernel != "generic":
            continue
        e = cov.setdefault((c.layout, c.mainloop, c.epilogue), set())
        if c.M % 128:
            e.add("M")
        if c.N % 128:
            e.add("N")
        if (c.K // 64) % 3 if c.mainloop == "ring" else c.K % 64:
            e.add("K")
    return cov


REQUIRED_ROUTES = {(("MN" if a else "K") + "x" + ("MN" if b else "K"), ml, ep)
                   for a, b in LAYOUTS for ml in ("ring", "register") for ep in ("staged", "direct")}

__all__ = ["CASES", "CASE_BY_NAME", "MAX_QUANTA", "GemmCase", "GemmData", "REQUIRED_ROUTES", "gemm_buffers", "gemm_data",
           "gemm_exactness_violations", "gemm_fp64", "gemm_kwargs", "gemm_mismatches", "gemm_pre_fp64",
           "operand_image", "rounding_census", "route_coverage", "to_bf16_fp64"]
