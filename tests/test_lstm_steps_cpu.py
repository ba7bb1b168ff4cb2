"""The per-step float64 LSTM reference (wellflow/train/lstm_ref.py) proved without a GPU:
its layout decoders against per-element loops written from csrc/lstm_layout.h, an fp32
emulation of the kernels' arithmetic that must pass every check with the caps asserted, and
nine mutations of the emulated device state that must each be rejected where they were made.
The calls training and scoring make are proved the same way: the emulation adds into a preset
bucket and loss accumulator (``prior=``), reads its batch through a window table (``rows=``) or
runs a short inference batch (``short=``), and ten more mutations of those calls are each
rejected at their site; the prior itself is shown to have teeth (test_prior_has_teeth).
tests/test_lstm_steps_gpu.py and tests/test_lstm_calls_gpu.py run the same checker on what the
kernels leave in memory."""
import pytest
import torch

from wellflow.data.synth import synth_lstm_batch
from wellflow.models.lstm import LstmLayout, init_lstm_flat
from wellflow.train import lstm_ref as R

import lstm_plans as P

BF = torch.bfloat16
SIG_SCALE = torch.tensor(-1.4426950408889634, dtype=torch.float32)  # csrc/common.h kLstmSigScale
TANH_SCALE = torch.tensor(2.8853900817779268, dtype=torch.float32)  # kLstmTanhScale


# ------------------------------------------------------------------ decoders vs slow loops
# (the inverse layouts: only the emulation below writes them)
def encode_fn(x: torch.Tensor) -> torch.Tensor:
    """[n][B][H] -> flat FN slabs (padding rows zero)."""
    n, B, H = x.shape
    out = torch.zeros(n, R.fn_rows(B) * H, dtype=x.dtype, device=x.device)
    out[:, R.fn_index(B, H, x.device)] = x
    return out.view(-1)


def encode_s(x: torch.Tensor) -> torch.Tensor:
    T, B, H, _ = x.shape
    out = torch.zeros(T, R.fn_rows(B) * 4 * H, dtype=x.dtype, device=x.device)
    out[:, R.s_index(B, H, x.device)] = x
    return out.view(-1)


def _fn_off(m, u, H):  # lstm_layout.h: block (m>>4, u>>4) row-major, lane ((m&15)>>2)*16 + (u&15), slot m&3
    return ((m >> 4) * (H >> 4) + (u >> 4)) * 256 + (((m & 15) >> 2) * 16 + (u & 15)) * 4 + (m & 3)


def _s_off(m, u, g, H):  # two 16-B halves per lane: rows 0-1 at lane*8, rows 2-3 at 512 + lane*8
    lane, r = ((m & 15) >> 2) * 16 + (u & 15), m & 3
    return ((m >> 4) * (H >> 4) + (u >> 4)) * 1024 + (512 if r >= 2 else 0) + lane * 8 + (r & 1) * 4 + g


@pytest.mark.parametrize("B", [16, 40, 48])
def test_decoders_match_slow_loops(B):
    H, T, KA = 128, 2, 192
    Bp, G = R.fn_rows(B), 4 * H
    assert Bp == (48 if B == 40 else B)
    cst = torch.arange((T + 1) * Bp * H, dtype=torch.float64)
    s = torch.arange(T * Bp * G, dtype=torch.float64)
    dC, dS = R.decode_fn(cst, B, H), R.decode_s(s, T, B, H)
    assert dC.shape == (T + 1, B, H) and dS.shape == (T, B, H, 4)
    okc = oks = True
    for m in range(B):
        for u in range(H):
            okc &= dC[1, m, u].item() == Bp * H + _fn_off(m, u, H)
            for g in range(4):
                oks &= dS[1, m, u, g].item() == Bp * G + _s_off(m, u, g, H)
    assert okc and oks
    # every offset used once, the padding rows never
    assert R.fn_index(B, H).unique().numel() == B * H and R.s_index(B, H).unique().numel() == B * G
    assert int(R.fn_index(B, H).max()) < Bp * H and int(R.s_index(B, H).max()) < Bp * G
    # encode is the inverse, padding rows zero
    x = torch.randn(T + 1, B, H)
    assert torch.equal(R.decode_fn(encode_fn(x), B, H), x)
    xs = torch.randn(T, B, H, 4)
    assert torch.equal(R.decode_s(encode_s(xs), T, B, H), xs)
    # dg_col = 4 u + gate (DG columns, WhhT columns, rows of W / gW); gate_col (Wp rows)
    dg = torch.arange(T * B * G, dtype=torch.float64)
    wh = torch.arange(H * G, dtype=torch.float64)
    w = torch.arange(G * KA, dtype=torch.float64)
    dDG, dWh, dW, dWp = R.decode_dg(dg, T, B, H), R.decode_whht(wh, H), R.decode_w_rows(w.view(G, KA), H), R.decode_wp(w, H, KA)
    ok = True
    for u in range(H):
        for g in range(4):
            ok &= dDG[1, B - 1, u, g].item() == (B + B - 1) * G + 4 * u + g
            ok &= dWh[5, u, g].item() == 5 * G + 4 * u + g
            ok &= dW[u, g, 7].item() == (4 * u + g) * KA + 7
            ok &= dWp[u, g, 7].item() == ((u >> 4) * 64 + g * 16 + (u & 15)) * KA + 7
    assert ok


# ------------------------------------------------------------------ fp32 emulation
def emulate(F, H, T, B, seed=0, loss="mse", mut=None, x_scale=1.0, prior=None, rows=None, short=None):
    """The kernels' arithmetic in plain float32 torch ops with the four bf16 roundings, filling
    the engine's buffers in the engine's layouts. ``mut``: one mutation (name, ...).
    ``prior`` = (bucket, loss accumulator): preset before the call, which adds to both
    (zero_grads=False, loss_into=). ``rows`` = (table, starts, yall, ids): the batch is read
    through a window table, ``x[b][t] = table[starts[ids[b]] + t]``, ``y = yall[ids]``.
    ``short`` = b: an inference call on the first b rows, the rest zero padding (``forward``)."""
    mut = mut or ("none",)
    lay = LstmLayout(F, H)
    KX, KA, G = lay.KX, lay.KA, lay.G
    params = init_lstm_flat(F, H, seed=seed)
    if rows is not None:
        table, starts, yall, ids = rows
        x, y = P.gather_windows(table, starts, ids, T) * x_scale, yall[ids]
    else:
        x, y = synth_lstm_batch(B, T, F, seed=seed)
        x, y = x.float() * x_scale, y.float()
    x_read, y_read = x, y  # what the emulated device reads; x, y stay what the caller asked for
    if mut[0] == "y_first_rows":  # the targets of windows 0 .. B-1, not of windows ids
        y_read = yall[:B]
    if mut[0] == "ids_slip":  # row k packed from window ids[k - 1]
        x_read = x.clone()
        x_read[mut[1]] = x[mut[1] - 1]
    if short is not None:
        x = x.clone()
        x[short:] = 0.0
        x_read = x
        if mut[0] == "pad_stale":  # a padding row still holds the previous call's window
            x_read = x.clone()
            x_read[mut[1]] = synth_lstm_batch(B, T, F, seed=seed)[0][mut[1]].float() * x_scale
    gs = 1.0 / B
    W, w_out, b_out = lay.views(params)
    scale = torch.stack([SIG_SCALE, SIG_SCALE, TANH_SCALE, SIG_SCALE])
    gc = R.gate_col_index(H)
    Wp = torch.zeros(G, KA, dtype=BF)
    Wp[gc] = (W.view(H, 4, KA) * scale[None, :, None]).to(BF)
    WhhT = W[:, KX:].to(BF).t().contiguous()
    XH = torch.zeros(T + 1, B, KA, dtype=BF)
    XH[:T, :, :KX] = R.pack_x_ref(x_read, KX)
    if mut[0] == "h0":  # a stray store into h_{-1}; every step below follows it, as a device would
        XH[0, mut[1], KX + mut[2]] = 2.0 ** -6
    S = torch.zeros(T, B, H, 4, dtype=BF)
    Cst = torch.zeros(T + 1, B, H, dtype=BF)
    c = torch.zeros(B, H)
    one, two = torch.tensor(1.0), torch.tensor(2.0)
    for t in range(T):
        z = (XH[t].float() @ Wp.float().t())[:, gc]
        if mut[0] == "kslice" and t == mut[1]:  # one 64-column k-slice missing for one 16-row block
            rows, k0 = slice(mut[2], mut[2] + 16), mut[3]
            z[rows] -= (XH[t, rows, k0:k0 + 64].float() @ Wp[:, k0:k0 + 64].float().t())[:, gc]
        if mut[0] == "swap_if":
            z[:, mut[1], [0, 1]] = z[:, mut[1], [1, 0]]
        p = torch.exp2(z)
        i, f, o = one / (one + p[..., 0]), one / (one + p[..., 1]), one / (one + p[..., 3])
        g = one - two / (p[..., 2] + one)
        c = f * c + i * g
        S[t] = torch.stack([i, f, g, o], -1).to(BF)
        Cst[t + 1] = c.to(BF)
        XH[t + 1, :, KX:] = (o * torch.tanh(c)).to(BF)
        if mut[0] == "bf16_carry":
            c = c.to(BF).float()
        if mut[0] == "stale_h" and t == mut[1]:  # a 16-row block's h from the previous step
            rows = slice(mut[2], mut[2] + 16)
            XH[t + 1, rows, KX:] = XH[t, rows, KX:]
    hT = XH[T, :, KX:].float()
    pred = hT @ w_out + b_out
    dy, terms = R.loss_dy_ref(pred, y_read, gs, loss, 6.0)
    grads0, loss0 = (None, None) if prior is None else (prior[0].clone(), prior[1].clone().view(1))
    grads = torch.zeros(lay.numel) if prior is None else grads0.clone()
    gW, gw_out, gb_out = lay.views(grads)
    gw_out.add_(dy @ hT)
    gb_out.add_(dy.sum().view(1))
    loss_sum = terms.sum().float().view(1) + (0.0 if prior is None else loss0)
    DG = torch.zeros(T, B, H, 4, dtype=BF)
    k = torch.zeros(B, H)
    if mut[0] == "carry_T1":
        k[mut[1]:mut[1] + 16] = 0.01
    for t in range(T - 1, -1, -1):
        dh = dy[:, None] * w_out[None, :] if t == T - 1 else DG[t + 1].view(B, G).float() @ WhhT.float().t()
        if mut[0] == "row_slip" and t == mut[1]:
            dh[mut[2]] = dh[mut[2] + 1].clone()
        i, f, g, o = S[t].float().unbind(-1)
        cp = Cst[t].float()
        tc = torch.tanh(f * cp + i * g)
        dc = k + dh * o * (one - tc * tc)
        k = dc * f
        DG[t] = torch.stack([dc * g * i * (one - i), dc * cp * f * (one - f), dc * i * (one - g * g),
                             dh * tc * o * (one - o)], -1).to(BF)
    steps = [t for t in range(T) if not (mut[0] == "gw_skip_t" and t == mut[1])]
    gW.add_(sum(DG[t].view(B, G).float().t() @ XH[t].float() for t in steps))
    p0 = lay.views(grads0) if prior is not None else None
    if mut[0] == "gw_store":  # the sum stored over the prior, one element or a whole tile
        _, r, c = mut
        gW[r, c] -= p0[0][r, c]
    if mut[0] == "gwout_store":
        gw_out.sub_(p0[1])
    if mut[0] == "gbout_store":
        gb_out.sub_(p0[2])
    if mut[0] == "loss_store":
        loss_sum = terms.sum().float().view(1)
    if mut[0] == "gw_pad_zeroed":
        gW[mut[1], mut[2]] = 0.0
    if mut[0] == "gw_pad":
        gW[mut[1], mut[2]] = 1e-6
    if mut[0] == "s_2ulp":
        _, t, m, u, gate = mut
        v = S[t, m, u, gate].float()
        S[t, m, u, gate] = (v + 2 * 2.0 ** (torch.frexp(v.abs())[1].item() - 1 - 7)).to(BF)  # bf16 ulp = 2^(e-7)
        assert S[t, m, u, gate].float() != v
    return R.LstmState(F, H, T, B, XH.view(-1), Wp.view(-1), WhhT.view(-1), encode_fn(Cst), encode_s(S),
                       DG.view(-1), pred, dy, loss_sum, grads, params, x, y, gs, loss, 6.0, grads0, loss0)


CASES = [(64, 128, 5, 16), (40, 128, 4, 9), (64, 512, 3, 127)]
_clean = {}


def _clean_checks(case):
    if case not in _clean:
        B, H, T, F = case
        _clean[case] = R.check_all(emulate(F, H, T, B))  # raises CapExceeded if a cap is missed
    return _clean[case]


@pytest.mark.parametrize("case", CASES)
def test_fp32_emulation_passes_every_check_under_the_caps(case):
    checks = _clean_checks(case)
    assert not R.violations(checks), R.describe(checks)
    B, H, T, F = case
    names = [c.name for c in checks]
    assert names.count("S") == T and names.count("Cst") == T and names.count("h") == T and names.count("DG") == T
    assert {"Cst0", "xblock", "h_init", "pred", "dy", "loss_sum", "gw_out", "gb_out", "gW", "gW_pad"} <= set(names)
    for c in checks:  # the caps, as the checker asserted them (lstm_ref._cap)
        if c.name in ("S", "Cst", "h"):
            assert c.max_slack <= 2.0 ** -10, (c.name, c.t, c.max_slack)
        assert c.worst <= 1.0
    print(case, R.summary(checks))


def test_mae_clip_head_passes():
    st = emulate(16, 128, 3, 64, loss="mae_clip")
    checks = R.check_all(st)
    assert not R.violations(checks), R.describe(checks)


def test_caps_are_asserted_by_the_checker():
    """Inputs 64 times wider push the pre-activation bound over 2^-10: the checker refuses."""
    with pytest.raises(R.CapExceeded):
        R.check_forward(emulate(127, 512, 2, 64, x_scale=64.0))


def _viol(mut, case=(64, 128, 5, 16), **kw):
    B, H, T, F = case
    st = emulate(F, H, T, B, mut=mut, **kw)
    return R.violations(R.check_all(st))


def test_mutation_s_element_two_ulps():
    v = _viol(("s_2ulp", 2, 37, 101, 3))
    s = [w for w in v if w[0] == "S"]
    assert [w[:5] for w in s] == [("S", 2, 37, 101, 3)], v
    assert s[0][5] > 1.5  # 2 ulps = 4 half ulps, minus at most one rounding
    # the emulated DG came from the unmutated gate: the same (row, unit), from that step down (the dc carry)
    assert all(w[1] <= 2 and w[2:4] == (37, 101) for w in v if w[0] == "DG") and all(w[0] in ("S", "DG") for w in v)


def test_mutation_missing_k_slice():
    v = _viol(("kslice", 1, 16, 64))
    # S at that step alone; the c carry is not in memory, so the reference chains its own and
    # the same rows stay wrong in Cst / h afterwards
    assert v and all(16 <= w[2] < 32 and w[0] in ("S", "Cst", "h") and w[1] >= 1 for w in v), v
    assert {w[1] for w in v if w[0] == "S"} == {1}
    assert len({w[2] for w in v if w[0] == "S"}) == 16  # every row of the block


def test_mutation_c_carried_in_bf16():
    v = _viol(("bf16_carry",))
    assert v and all(w[0] in ("Cst", "h") and w[1] >= 1 for w in v), v
    assert any(w[0] == "Cst" for w in v)


def test_mutation_i_f_gates_swapped():
    v = _viol(("swap_if", 77))
    assert all(w[0] in ("S", "Cst", "h") and w[3] == 77 for w in v), v
    assert {w[1] for w in v if w[0] == "S"} == set(range(5))
    assert {w[4] for w in v if w[0] == "S"} == {0, 1}


def test_mutation_stale_hand_off():
    v = _viol(("stale_h", 2, 32))
    assert v and all(w[0] == "h" and w[1] == 2 and 32 <= w[2] < 48 for w in v), v
    assert len({w[2] for w in v}) == 16


def test_mutation_row_off_slip():
    v = _viol(("row_slip", 3, 21))
    assert v and all(w[0] == "DG" and w[1] <= 3 and w[2] == 21 for w in v), v


def test_mutation_dc_carry_not_zero_at_last_step():
    v = _viol(("carry_T1", 16))
    assert v and all(w[0] == "DG" and 16 <= w[2] < 32 for w in v), v
    assert any(w[1] == 4 for w in v)


def test_mutation_timestep_missing_from_gw():
    v = _viol(("gw_skip_t", 1))
    assert v and all(w[0] == "gW" for w in v), v


def test_mutation_gw_padding_column():
    v = _viol(("gw_pad", 301, 40))
    assert sorted(w[:4] for w in v) == [("gW", -1, 301, 40), ("gW_pad", -1, 301, 40 - 17)], v


# ------------------------------------------------------------------ the calls training and scoring make
def _prior(case):
    B, H, T, F = case
    return P.lattice_prior(LstmLayout(F, H)), torch.tensor([P.LOSS0])


def _rows(case, which=0):
    B, H, T, F = case
    table, starts, yall, ids = P.window_rows(B, T, F)
    return table, starts, yall, ids[which]


@pytest.mark.parametrize("case", CASES)
def test_emulation_with_a_prior_and_rows_passes_every_check(case):
    """The accumulating call (bucket and loss accumulator preset, zero_grads=False, loss_into=) and
    the row-indexed call, each alone and both at once, under the same caps."""
    B, H, T, F = case
    for kw in (dict(prior=_prior(case)), dict(rows=_rows(case)), dict(prior=_prior(case), rows=_rows(case, 1))):
        st = emulate(F, H, T, B, **kw)
        checks = R.check_all(st)  # raises CapExceeded if a cap is missed
        assert not R.violations(checks), R.describe(checks)
        assert all(c.worst <= 1.0 for c in checks)
        assert {"h_init", "gW", "gW_pad", "gw_out", "gb_out", "loss_sum", "xblock"} <= {c.name for c in checks}
        if "prior" in kw:  # the prior really is in what was checked
            assert st.grads0 is not None and st.loss_sum.item() > P.LOSS0
            assert torch.equal(st.views(st.grads)[0][:, F + 1:st.KX], st.views(st.grads0)[0][:, F + 1:st.KX])
    # rows: two windows are in the batch twice, and the windows overlap
    ids = _rows(case)[3]
    assert ids.unique().numel() == B - 2


@pytest.mark.parametrize("case", CASES)
def test_prior_has_teeth(case):
    """The lattice prior (lstm_plans.PRIOR_EXP) against the bound it enters, both from the float64
    side of the emulated call: every |prior| element is above 4x the bound at its element, so a
    dropped prior is a violation at every element of the bucket and of the accumulator (error >=
    |prior| - bound > 3 bounds), and the prior's largest rounding term ``n u |prior|`` is below the
    gradient's term ``n u sum|terms|`` at the median element, so the bound is still the gradient's.
    On CASES the gW window is one binade wide: the first condition needs |prior| > 2.6e-5 (the
    largest 4 n u sum|terms|, at (64, 128, 5, 16)), the second max |prior| < 8.8e-5 (the smallest
    median sum|terms| over all of gW, padding columns included, at (40, 128, 4, 9)): 2^-15 <= |prior|
    < 2^-14. gw_out: 1.8e-5 and 0.11, 2^-6; gb_out: 1.4e-4 and 2.0, 2^-4; the accumulator's 3.0
    against loss sums of 56 to 107."""
    B, H, T, F = case
    st = emulate(F, H, T, B, prior=_prior(case))
    items = dict(R.head_terms(st), gW=R.dw_terms(st))
    for name, (p, s, a, n) in items.items():
        assert bool((p != 0).all()), name
        bound = n * R.U32 * (p.abs() + a)
        assert bool((p.abs() > 4 * bound).all()), (name, float((bound / p.abs()).max()))
        assert float((n * R.U32 * p.abs()).max()) < float((n * R.U32 * a).median()), name
    lo, hi = 2.0 ** P.PRIOR_EXP["gW"], 2.0 ** (P.PRIOR_EXP["gW"] + 1)
    gW0 = st.views(st.grads0)[0].abs()
    assert bool((gW0 >= lo).all()) and bool((gW0 < hi).all())
    assert bool(((gW0 * 2.0 ** (12 - P.PRIOR_EXP["gW"])) % 1 == 0).all())  # the 2^-12 lattice of its binade


def _viol_prior(mut, case=(64, 128, 5, 16)):
    B, H, T, F = case
    return R.check_all(emulate(F, H, T, B, mut=mut, prior=_prior(case)))


def test_mutation_gw_element_stored_not_added():
    v = R.violations(_viol_prior(("gw_store", 301, 100)))
    assert [w[:4] for w in v] == [("gW", -1, 301, 100)], v
    assert v[0][4] > 3.0  # |prior| > 4 bounds, minus at most one


def test_mutation_gw_tile_stored_not_added():
    """A whole 256x288 tile (rows 256..511, columns 288..575 of the 2048x640 gW) stored over the prior."""
    checks = _viol_prior(("gw_store", slice(256, 512), slice(288, 576)), case=(64, 512, 3, 127))
    bad = [c for c in checks if c.count]
    assert [c.name for c in bad] == ["gW"] and bad[0].count == 256 * 288, R.describe(checks)
    ix = bad[0].idx
    assert int(ix[:, 0].min()) == 256 and int(ix[:, 0].max()) <= 511 and int(ix[:, 1].min()) == 288 and int(ix[:, 1].max()) == 575
    assert float(bad[0].ratio.min()) > 3.0


def test_mutation_prior_dropped_from_gw_out():
    v = R.violations(_viol_prior(("gwout_store",)))
    assert sorted(w[:3] for w in v) == [("gw_out", -1, u) for u in range(128)], v
    assert min(w[3] for w in v) > 3.0


def test_mutation_prior_dropped_from_gb_out():
    v = R.violations(_viol_prior(("gbout_store",)))
    assert [w[:3] for w in v] == [("gb_out", -1, 0)] and v[0][3] > 3.0, v


def test_mutation_loss_stored_not_added():
    v = R.violations(_viol_prior(("loss_store",)))
    assert [w[:3] for w in v] == [("loss_sum", -1, 0)] and v[0][3] > 3.0, v


def test_mutation_gw_padding_column_lost_its_prior():
    v = R.violations(_viol_prior(("gw_pad_zeroed", 301, 40)))
    assert sorted(w[:4] for w in v) == [("gW", -1, 301, 40), ("gW_pad", -1, 301, 40 - 17)], v


def test_mutation_h_init_not_zero():
    """One element of h_{-1} nonzero: ``h_init`` and nothing else. The emulated step 0 read it (row
    37's gates differ from the clean run's), and the step checks follow the device's own XH[0]."""
    B, H, T, F = 64, 128, 5, 16
    st = emulate(F, H, T, B, mut=("h0", 37, 101))
    v = R.violations(R.check_all(st))
    assert [w[:4] for w in v] == [("h_init", 0, 37, 101)], v
    S, S0 = R.decode_s(st.S, T, B, H), R.decode_s(emulate(F, H, T, B).S, T, B, H)
    assert not torch.equal(S[0, 37], S0[0, 37]) and torch.equal(S[0, 36], S0[0, 36])


def test_mutation_targets_of_the_first_rows():
    """y taken as yall[:B], not yall[ids]: dy at every row whose two targets differ, and the loss."""
    case = (64, 128, 5, 16)
    B, H, T, F = case
    rows = _rows(case)
    yall, ids = rows[2], rows[3]
    v = R.violations(R.check_all(emulate(F, H, T, B, mut=("y_first_rows",), rows=rows)))
    assert {w[0] for w in v} == {"dy", "loss_sum"}, v
    assert sorted(w[2] for w in v if w[0] == "dy") == (yall[:B] != yall[ids]).nonzero().view(-1).tolist()


def test_mutation_window_id_of_the_row_before():
    case = (64, 128, 5, 16)
    B, H, T, F = case
    v = R.violations(R.check_all(emulate(F, H, T, B, mut=("ids_slip", 21), rows=_rows(case))))
    assert v and all(w[0] == "xblock" and w[3] == 21 and w[4] < F for w in v), v
    assert {w[2] for w in v} == set(range(T))


def test_mutation_padding_row_keeps_the_previous_window():
    """A short inference batch (forward pads it with zero rows): row 50 of 64 still holds x."""
    B, H, T, F = 64, 128, 5, 16
    clean = R.check_inference(emulate(F, H, T, B, short=40))
    assert not R.violations(clean) and [c.name for c in clean][-2:] == ["h_init", "pred"]
    assert not {"dy", "loss_sum", "gW", "DG"} & {c.name for c in clean}
    v = R.violations(R.check_inference(emulate(F, H, T, B, short=40, mut=("pad_stale", 50))))
    assert v and all(w[0] == "xblock" and w[3] == 50 and w[4] < F for w in v), v
