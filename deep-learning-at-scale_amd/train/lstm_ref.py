"""Float64 reference of ONE LSTM step at a time, with worst-case fp32 error bounds.

Every LSTM kernel path (csrc/lstm.hip, lstm_persistent_fwd.inc.h, lstm_persistent_bwd.inc.h)
is a bf16 x bf16 -> fp32 GEMM followed by a pointwise fp32 epilogue, and all of them round to
bf16 in the same four places: the saved gates ``S``, the cell-state history ``Cst`` (the carry
itself stays fp32), the h block of ``XH`` (``bf16(o * tanh(c))`` from the fp32 ``o`` and ``c``)
and the gate gradients ``DG`` (the dc carry stays fp32). Every step's inputs and outputs stay
in device memory, so each step is checked on its own: the float64 value is computed from the
DEVICE's inputs to that step, and a correct kernel must have stored its bf16 neighbour,

    |dev - ref| <= half a bf16 ulp of ref + slack,

where ``slack`` bounds what fp32 arithmetic can move the value before the rounding. Nothing
compounds over T except the two fp32 carries (c forward, dc backward), which never reach
memory between steps; they and their bounds are chained here in float64.

How the slack is derived (unit ``u = 2^-23`` per fp32 operation: twice round-to-nearest's
unit, the margin for the MFMA's undocumented internal summation order and rounding):

* a dot product of n terms, summed in any order:  ``n u sum_k |a_k w_k|`` (a second matmul of
  absolute values);
* v_exp_f32 / v_rcp_f32: 1 ulp = relative ``u`` each (csrc/common.h);
* sigmoid gate from the scaled pre-activation z (Wp carries -log2 e):  s = 1 / (1 + 2^z).
  |ds/dz| = ln2 s (1 - s) <= ln2 / 4, and exp2, the add and the rcp each move s by at most
  ``u s``:  ``e_s = e_z ln2 / 4 + 3 u s``;
* tanh gate (Wp carries 2 log2 e):  g = 1 - 2 r, r = 1 / (2^z + 1).  |dg/dz| <= ln2 / 2; r
  carries 3 u r, doubled by the factor 2, and the subtraction rounds once:
  ``e_g = e_z ln2 / 2 + 6 u r + u |g|``;
* c = f c' + i g with the carry bound E':  ``E = (f + e_f) E' + |c'| e_f + (|g| + e_g) e_i +
  i e_g + 2 u (|f c'| + |i g|)`` (product and sum roundings, fused or not);
* tanh(c) = 1 - 2 / (exp(2c) + 1) with exp(x) = 2^(x log2 e): the scaling multiply moves the
  exponential by ``2 |c| u`` relative, exp2 / add / rcp by ``u`` each:
  ``e_tc = e_c + 2 r (3 + 2 |c|) u + u |tc|`` (|d tanh| <= 1);
* h = o tc:  ``e_h = o e_tc + |tc| e_o + e_o e_tc + u |h|``;
* backward (cell_bwd4): the inputs S, c_{t-1} are bf16 values read exactly; x = f c' + i g
  carries ``2 u (|f c'| + |i g|)``, q = 1 - tc^2 carries ``2 |tc| e_tc + 2 u``,
  dc = k + dh o q carries ``E_k + |o q| e_dh + |dh o| e_q + 3 u |dh o q| + u |dc|``, and each
  gate gradient ``dc * a * s (1 - s)`` carries ``e_dc |a s (1 - s)| + 6 u |dc a s|`` — the
  last term covers both the product form of lstm.hip and the ``p - p s`` form of the
  persistent kernel (three products, one subtraction of magnitudes <= |dc a s|).

``gate_col_index``, ``pack_x_ref`` and ``loss_dy_ref`` are shared by this checker and by the CPU
emulation in tests/test_lstm_steps_cpu.py; they are pinned independently of both by that file's
per-element decoder loops and by tests/test_lstm_pack_gpu.py (device packs, bit for bit).

The caps below are CONDITIONS on the inputs, not measurements: where the slack reaches them the
check has lost its teeth, so the checker refuses instead of passing.
"""
from __future__ import annotations

import dataclasses
import math

import torch

U32 = 2.0 ** -23
LN2 = math.log(2.0)
CAP_FWD = 2.0 ** -10   # absolute, S / Cst / h
CAP_DG = 2.0 ** -8     # x max |ref DG[t]|
CAP_GW = 2.0 ** -10    # x max |ref gW|, cases with T * B <= 1024
KEEP = 65536          # violations recorded per check (the count is always complete)


class CapExceeded(AssertionError):
    """The derived slack of a check is above its cap on these inputs (change the inputs)."""


# ---------------------------------------------------------------------------- layouts
def fn_rows(B: int) -> int:
    return (B + 15) & ~15


def _mu(B, H, device):
    m = torch.arange(B, device=device)[:, None]
    u = torch.arange(H, device=device)[None, :]
    blk = (m >> 4) * (H >> 4) + (u >> 4)
    lane = ((m & 15) >> 2) * 16 + (u & 15)
    return m, blk, lane


def fn_index(B: int, H: int, device=None) -> torch.Tensor:
    """[B][H] offsets of element (m, u) in one fragment-native slab (csrc/lstm_layout.h)."""
    m, blk, lane = _mu(B, H, device)
    return blk * 256 + lane * 4 + (m & 3)


def s_index(B: int, H: int, device=None) -> torch.Tensor:
    """[B][H][4] bf16 offsets of gates i, f, g, o of (m, u) in one S slab: 1024 per block, rows
    0-1 of a lane's four at lane * 8, rows 2-3 at kFnSHalf + lane * 8."""
    m, blk, lane = _mu(B, H, device)
    base = blk * 1024 + ((m & 3) >> 1) * 512 + lane * 8 + (m & 1) * 4
    return base[..., None] + torch.arange(4, device=device)


def gate_col_index(H: int, device=None) -> torch.Tensor:
    """[H][4]: forward gate column / Wp row of (unit, gate)."""
    u = torch.arange(H, device=device)[:, None]
    g = torch.arange(4, device=device)[None, :]
    return (u >> 4) * 64 + g * 16 + (u & 15)


def decode_fn(flat: torch.Tensor, B: int, H: int) -> torch.Tensor:
    """FN slabs (Cst: T + 1 of them, dcarry: one) -> [n][B][H]."""
    return flat.view(-1, fn_rows(B) * H)[:, fn_index(B, H, flat.device)]


def decode_s(flat: torch.Tensor, T: int, B: int, H: int) -> torch.Tensor:
    """S -> [T][B][H][4], gates i, f, g, o."""
    return flat.view(T, fn_rows(B) * 4 * H)[:, s_index(B, H, flat.device)]


def decode_dg(flat: torch.Tensor, T: int, B: int, H: int) -> torch.Tensor:
    """DG (columns dg_col = 4 u + gate) -> [T][B][H][4]."""
    return flat.view(T, B, H, 4)


def decode_whht(flat: torch.Tensor, H: int) -> torch.Tensor:
    """WhhT [H][G] (columns dg_col) -> [k][u][gate] = W_hh[(u, gate)][k]."""
    return flat.view(H, H, 4)


def decode_w_rows(W: torch.Tensor, H: int) -> torch.Tensor:
    """Master W / gW [G][KA] (rows dg_col) -> [u][gate][KA]."""
    return W.reshape(H, 4, -1)


def decode_wp(flat: torch.Tensor, H: int, KA: int) -> torch.Tensor:
    """Wp [G][KA] (rows gate_col) -> [u][gate][KA]."""
    return flat.view(4 * H, KA)[gate_col_index(H, flat.device)]


# ---------------------------------------------------------------------------- one step
def _tanh_ref(c, e_c):
    tc = torch.tanh(c)
    r = 1.0 / (torch.exp(2.0 * c) + 1.0)
    return tc, e_c + 2.0 * r * (3.0 + 2.0 * c.abs()) * U32 + U32 * tc.abs()


def fwd_step_ref(xh_t, Wp, c_prev, E_prev):
    """xh_t [B][KA] and Wp [G][KA] as the device holds them (bf16 values), c_prev / E_prev
    [B][H] float64: the chained carry and its bound. Returns a dict of float64 tensors:
    S, e_S [B][H][4]; c, E, h, e_h [B][H]."""
    xh, W = xh_t.double(), Wp.double()
    G, KA = W.shape
    gc = gate_col_index(G // 4, W.device)
    z = (xh @ W.t())[:, gc]
    e_z = KA * U32 * (xh.abs() @ W.abs().t())[:, gc]
    p = torch.exp2(z)
    S = 1.0 / (1.0 + p)
    e_S = e_z * (LN2 / 4) + 3 * U32 * S
    r = 1.0 / (p[..., 2] + 1.0)
    S[..., 2] = 1.0 - 2.0 * r
    e_S[..., 2] = e_z[..., 2] * (LN2 / 2) + 6 * U32 * r + U32 * S[..., 2].abs()
    i, f, g, o = S.unbind(-1)
    e_i, e_f, e_g, e_o = e_S.unbind(-1)
    c = f * c_prev + i * g
    E = ((f + e_f) * E_prev + c_prev.abs() * e_f + (g.abs() + e_g) * e_i + i * e_g
         + 2 * U32 * ((f * c_prev).abs() + (i * g).abs()))
    tc, e_tc = _tanh_ref(c, E)
    h = o * tc
    e_h = o * e_tc + tc.abs() * e_o + e_o * e_tc + U32 * h.abs()
    return {"S": S, "e_S": e_S, "c": c, "E": E, "h": h, "e_h": e_h}


def dh_ref(dg_next, WhhT):
    """dh = DG[t+1] @ W_hh from the device's DG[t+1] [B][G] and WhhT [H][G], and its bound."""
    a, w = dg_next.double(), WhhT.double()
    return a @ w.t(), a.shape[1] * U32 * (a.abs() @ w.abs().t())


def bwd_step_ref(S_t, c_prev, dh, e_dh, k, E_k):
    """cell_bwd4 in float64. S_t [B][H][4] and c_prev [B][H]: the device's bf16 gates and
    c_{t-1}; dh, e_dh: this step's dh and its bound; k, E_k: the chained dc carry. Returns
    DG, e_DG [B][H][4] and the next carry k, E_k."""
    i, f, g, o = S_t.double().unbind(-1)
    cp = c_prev.double()
    x = f * cp + i * g
    tc, e_tc = _tanh_ref(x, 2 * U32 * ((f * cp).abs() + (i * g).abs()))
    q = 1.0 - tc * tc
    e_q = 2 * tc.abs() * e_tc + 2 * U32
    dho = dh * o
    dc = k + dho * q
    e_dc = E_k + (o * q).abs() * e_dh + dho.abs() * e_q + 3 * U32 * (dho * q).abs() + U32 * dc.abs()
    kn = dc * f
    E_kn = f * e_dc + U32 * kn.abs()
    DG = torch.stack([dc * g * i * (1 - i), dc * cp * f * (1 - f), dc * i * (1 - g * g),
                      dh * tc * o * (1 - o)], -1)
    e_DG = torch.stack([
        e_dc * (g * i * (1 - i)).abs() + 6 * U32 * (dc * g * i).abs(),
        e_dc * (cp * f * (1 - f)).abs() + 6 * U32 * (dc * cp * f).abs(),
        e_dc * (i * (1 - g * g)).abs() + 6 * U32 * (dc * i).abs(),
        (e_dh * tc.abs() + dh.abs() * e_tc + e_dh * e_tc) * (o * (1 - o)) + 6 * U32 * (dh * tc * o).abs()], -1)
    return DG, e_DG, kn, E_kn


# ---------------------------------------------------------------------------- comparison
@dataclasses.dataclass
class Check:
    name: str
    t: int
    count: int
    idx: torch.Tensor      # [n][ndim] indices of the violations within this tensor
    ratio: torch.Tensor    # [n] err / (half ulp + slack) of the violations
    worst: float           # largest ratio over every element
    share: float           # median slack / half ulp over the elements with a nonzero half ulp
    max_slack: float

    def where(self):
        """Violations as tuples (t, *index)."""
        return [(self.t, *map(int, r)) for r in self.idx.tolist()]


def bf16_half_ulp(ref: torch.Tensor) -> torch.Tensor:
    """2^(floor(log2 |ref|) - 8); 0 at ref = 0."""
    a = ref.abs()
    _, ex = torch.frexp(a)  # a = m 2^ex, m in [0.5, 1): floor(log2 a) = ex - 1
    return torch.where(a > 0, torch.exp2((ex - 9).double()), torch.zeros_like(a))


def within_bf16(dev, ref, slack, name="", t=-1) -> Check:
    """|dev - ref| <= half a bf16 ulp of ref + slack at every element, or the violations. The
    half ulp is that of ref's own binade: where the fp32 value crosses into the binade above,
    it lies within slack of the power of two and rounds onto it as long as slack is below that
    half ulp, so the error stays under slack alone."""
    dev, ref = dev.double(), ref.double()
    slack = torch.as_tensor(slack, dtype=torch.float64, device=ref.device).expand_as(ref)
    return _compare(dev, ref, bf16_half_ulp(ref), slack, name, t)


def within_abs(dev, ref, slack, name="", t=-1) -> Check:
    """|dev - ref| <= slack (fp32 outputs: no bf16 rounding)."""
    dev, ref = dev.double(), ref.double()
    slack = torch.as_tensor(slack, dtype=torch.float64, device=ref.device).expand_as(ref)
    return _compare(dev, ref, torch.zeros_like(ref), slack, name, t)


def _compare(dev, ref, half, slack, name, t):
    allow = half + slack
    err = (dev - ref).abs()
    bad = ~(err <= allow)  # a NaN is a violation
    ratio = torch.where(allow > 0, err / allow.clamp_min(1e-300),
                        torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, math.inf), ratio)
    nz = half > 0
    share = float((slack[nz] / half[nz]).median()) if bool(nz.any()) else 0.0
    idx = bad.nonzero()
    return Check(name, t, int(idx.shape[0]), idx[:KEEP].cpu(), ratio[bad][:KEEP].cpu(),
                 float(ratio.max()) if ratio.numel() else 0.0, share,
                 float(slack.max()) if slack.numel() else 0.0)


# ---------------------------------------------------------------------------- whole state
@dataclasses.dataclass
class LstmState:
    """Everything a forward_backward leaves in device memory, as flat tensors in the engine's
    layouts (CPU or GPU), plus the inputs. ``grads`` is the flat gradient buffer."""
    F: int
    H: int
    T: int
    B: int
    XH: torch.Tensor
    Wp: torch.Tensor
    WhhT: torch.Tensor
    Cst: torch.Tensor
    S: torch.Tensor
    DG: torch.Tensor
    pred: torch.Tensor
    dy: torch.Tensor
    loss_sum: torch.Tensor
    grads: torch.Tensor
    params: torch.Tensor
    x: torch.Tensor
    y: torch.Tensor
    grad_scale: float
    loss: str = "mse"
    clip: float = 6.0
    grads0: torch.Tensor | None = None   # the flat bucket before the call (None: zero)
    loss0: torch.Tensor | None = None    # the loss accumulator before the call (None: zero)

    @property
    def KX(self):
        return (self.F + 1 + 63) // 64 * 64

    @property
    def KA(self):
        return self.KX + self.H

    def views(self, flat):
        G, KA, H = 4 * self.H, self.KA, self.H
        return flat[: G * KA].view(G, KA), flat[G * KA: G * KA + H], flat[G * KA + H: G * KA + H + 1]

    def prior(self):
        """(gW0, gw_out0, gb_out0, loss0): what the bucket and the loss accumulator held before
        the call, zeros where none was given."""
        g0 = self.grads0 if self.grads0 is not None else torch.zeros_like(self.grads)
        l0 = self.loss0 if self.loss0 is not None else torch.zeros_like(self.loss_sum)
        return (*self.views(g0), l0.view(1))

    @classmethod
    def of_engine(cls, eng, x, y, grad_scale, grads0=None, loss0=None, loss_acc=None):
        """Snapshot (clones) of a NativeLSTM after forward_backward(x, y, grad_scale). ``grads0`` /
        ``loss0``: the bucket and the accumulator as they were before a call that added to them
        (zero_grads=False, loss_into=loss_acc); ``loss_acc``: the tensor that received the loss
        (the engine's own ``loss_sum`` when None)."""
        c = lambda v: v.detach().clone()
        o = lambda v: None if v is None else c(v).view(-1)
        return cls(eng.F, eng.H, eng.T, eng.B, c(eng.XH), c(eng.Wp), c(eng.WhhT), c(eng.Cst), c(eng.S),
                   c(eng.DG), c(eng.pred), c(eng.dy), c(eng.loss_sum if loss_acc is None else loss_acc).view(-1),
                   c(eng.grads), c(eng.params), c(x), c(y), float(grad_scale), eng.loss_kind, float(eng.clip),
                   o(grads0), o(loss0))


def pack_x_ref(x: torch.Tensor, KX: int) -> torch.Tensor:
    """The x block of XH: [T][B][KX] bf16 = [bf16(x[b][t]) | 1 | 0 ...]."""
    B, T, F = x.shape
    out = torch.zeros(T, B, KX, dtype=torch.bfloat16, device=x.device)
    out[:, :, :F] = x.transpose(0, 1).to(torch.bfloat16)
    out[:, :, F] = 1.0
    return out


def _cap(chk: Check, cap: float, what: str):
    if not chk.max_slack <= cap:
        raise CapExceeded(f"{what}: slack {chk.max_slack:.3e} above its cap {cap:.3e}; the inputs are too "
                          f"wide for this check (scale the data, not the cap)")


def check_forward(st: LstmState) -> list:
    """S[t], Cst[t+1] and the h block of XH[t+1] for every t, each from XH[t] and Wp as the
    device left them; Cst slab 0, the x blocks and h before step 0 (``h_init``) exact."""
    T, B, H, KX, KA = st.T, st.B, st.H, st.KX, st.KA
    XH = st.XH.view(T + 1, B, KA)
    Wp = st.Wp.view(4 * H, KA)
    Cst = decode_fn(st.Cst, B, H)
    S = decode_s(st.S, T, B, H)
    out = []
    c = torch.zeros(B, H, dtype=torch.float64, device=XH.device)
    E = torch.zeros_like(c)
    z0 = torch.zeros_like(c)
    out.append(within_abs(Cst[0], z0, 0.0, "Cst0", 0))
    xref = pack_x_ref(st.x, KX)
    out.append(within_abs(XH[:T, :, :KX], xref, 0.0, "xblock", 0))
    out.append(within_abs(XH[T, :, :KX], torch.zeros(B, KX, dtype=torch.float64, device=XH.device), 0.0, "xblock", T))
    for t in range(T):
        r = fwd_step_ref(XH[t], Wp, c, E)
        c, E = r["c"], r["E"]
        for chk, what in ((within_bf16(S[t], r["S"], r["e_S"], "S", t), "S"),
                          (within_bf16(Cst[t + 1], c, E, "Cst", t), "Cst"),
                          (within_bf16(XH[t + 1, :, KX:], r["h"], r["e_h"], "h", t), "h")):
            _cap(chk, CAP_FWD, f"{what}[{t}]")
            out.append(chk)
    # h_{-1}: the h block of XH[0] is zeroed by the constructor and written by nothing after it;
    # step 0 above follows the device's own XH[0], so this is the only check a stray store there meets
    out.append(within_abs(XH[0, :, KX:], z0, 0.0, "h_init", 0))
    return out


def loss_dy_ref(pred, y, grad_scale, loss, clip):
    """dy (fp32, the kernels' own operation order on the device's pred) and the per-row loss
    terms in float64."""
    if loss == "mse":  # head kernels: dy = float(2 gs) * (pred - y)
        diff = pred - y
        return torch.tensor(2.0 * grad_scale, dtype=torch.float32, device=pred.device) * diff, diff.double() ** 2
    e = y - pred  # loss_kernel kind 1
    a = e.abs()
    d = torch.where(a <= clip, -torch.sign(e), torch.zeros_like(e))
    return d * torch.tensor(grad_scale, dtype=torch.float32, device=pred.device), a.clamp(max=clip).double()


def check_head(st: LstmState) -> list:
    """pred within the dot-product bound ``(H + 1) u (|h| . |w| + |b|)``; dy against the loss formula
    applied in fp32 to the device's own pred: exact for clipped MAE, within 2^-24 |dy| (at most one
    fp32 ulp) for MSE; loss_sum / gw_out / gb_out within their sum bounds ``n u sum|terms|``.
    With a prior (``grads0`` / ``loss0``) each of the three sums is ``prior + sum``: the prior is one
    more term of the same bound, and the adds that reach the word count as further roundings."""
    out = [check_pred(st)]
    dy, terms = loss_dy_ref(st.pred, st.y.float(), st.grad_scale, st.loss, st.clip)
    # dy: clipped MAE exactly (a sign times the scale, or 0: nothing rounds); MSE within 1 fp32
    # ulp, taken as 2^-24 relative (the spacing of fp32 numbers is at least that)
    e_dy = 0.0 if st.loss != "mse" else 2.0 ** -24 * dy.double().abs()
    out.append(within_abs(st.dy, dy, e_dy, "dy"))
    _, gw_out, gb_out = st.views(st.grads)
    for name, dev in (("loss_sum", st.loss_sum), ("gw_out", gw_out), ("gb_out", gb_out)):
        prior, s, a, n = head_terms(st)[name]
        out.append(within_abs(dev, prior + s, n * U32 * (prior.abs() + a), name))
    return out


def check_pred(st: LstmState) -> Check:
    T, B, H, KX, KA = st.T, st.B, st.H, st.KX, st.KA
    hT = st.XH.view(T + 1, B, KA)[T, :, KX:].double()
    _, w_out, b_out = st.views(st.params)
    w = w_out.double()
    pred = hT @ w + b_out.double()
    e_pred = (H + 1) * U32 * (hT.abs() @ w.abs() + b_out.double().abs())
    return within_abs(st.pred, pred, e_pred, "pred")


def head_adds(B: int) -> tuple:
    """Adds that reach (the loss word, a gw_out / gb_out word) on the loosest route: one atomic per
    workgroup, and no launcher starts more workgroups than rows. csrc/elementwise.hip: launch_loss
    caps its grid at 1024 blocks (launch_head_fwd at 512, launch_head_fwd_bwd at 128);
    launch_head_fwd_bwd and launch_head_bwd_w both cap theirs at 128."""
    return min(B, 1024), min(B, 128)


def head_terms(st: LstmState) -> dict:
    """name -> (prior, sum, sum of |terms|, n) of loss_sum, gw_out and gb_out in float64; the bound
    of each is ``n u (|prior| + sum|terms|)``. Without a prior n is the term count the bound always
    had; with one it grows by :func:`head_adds`."""
    T, B, KX, KA = st.T, st.B, st.KX, st.KA
    hT = st.XH.view(T + 1, B, KA)[T, :, KX:].double()
    _, terms = loss_dy_ref(st.pred, st.y.float(), st.grad_scale, st.loss, st.clip)
    d = st.dy.double()
    _, gw0, gb0, l0 = st.prior()
    nl, ng = head_adds(B)
    xl = nl if st.loss0 is not None else 0
    xg = ng if st.grads0 is not None else 0
    return {"loss_sum": (l0.double(), terms.sum().view(1), terms.sum().view(1), B + 4 + xl),
            "gw_out": (gw0.double(), d @ hT, d.abs() @ hT.abs(), B + 1 + xg),
            "gb_out": (gb0.double(), d.sum().view(1), d.abs().sum().view(1), B + xg)}


def check_backward(st: LstmState) -> list:
    """DG[t] for every t from the device's S[t], Cst[t], DG[t+1], WhhT (dy, w_out at T-1)."""
    T, B, H = st.T, st.B, st.H
    Cst = decode_fn(st.Cst, B, H)
    S = decode_s(st.S, T, B, H)
    DG = decode_dg(st.DG, T, B, H)
    WhhT = st.WhhT.view(H, 4 * H)
    _, w_out, _ = st.views(st.params)
    k = torch.zeros(B, H, dtype=torch.float64, device=DG.device)
    E_k = torch.zeros_like(k)
    out = []
    for t in range(T - 1, -1, -1):
        if t == T - 1:
            dh = st.dy.double()[:, None] * w_out.double()[None, :]
            e_dh = U32 * dh.abs()
        else:
            dh, e_dh = dh_ref(DG[t + 1].reshape(B, 4 * H), WhhT)
        ref, e, k, E_k = bwd_step_ref(S[t], Cst[t], dh, e_dh, k, E_k)
        chk = within_bf16(DG[t], ref, e, "DG", t)
        _cap(chk, CAP_DG * float(ref.abs().max()), f"DG[{t}]")
        out.append(chk)
    return out


def check_dw(st: LstmState) -> list:
    """gW against prior + sum_{t,b} DG^T XH of the device's own DG and XH; its padding columns
    equal the prior exactly (0 without one)."""
    F, KX = st.F, st.KX
    gW, _, _ = st.views(st.grads)
    prior, s, a, n = dw_terms(st)
    chk = within_abs(gW, prior + s, n * U32 * (prior.abs() + a), "gW")
    if st.T * st.B <= 1024:  # against the gradient alone: a prior must not raise the cap
        _cap(chk, CAP_GW * float(s.abs().max()), "gW")
    return [chk, within_abs(gW[:, F + 1: KX], prior[:, F + 1: KX], 0.0, "gW_pad")]


def dw_adds(T: int) -> int:
    """Adds that reach a gW word on the loosest route: one per split-K partial (atomics, or the
    slab reduce's ``out[i] += ...``) of every dW launch. models/lstm.py picks at most 32 splits
    (``min(32, K // 16384)``); the side-stream route launches ceil(T / chunk) chunks of
    ``max(1, splits * chunk // T)`` splits each, which is at most 2 * 32 where that quotient is
    at least one and at most T chunks of one split where it is not."""
    return max(64, T)


def dw_terms(st: LstmState) -> tuple:
    """(prior, sum, sum of |terms|, n) of gW in float64; the bound is ``n u (|prior| + sum|terms|)``.
    n = T B without a prior, as the bound always had; with one it grows by :func:`dw_adds`."""
    T, B, H, KA = st.T, st.B, st.H, st.KA
    A = st.DG.view(T * B, 4 * H).double()
    X = st.XH.view(T + 1, B, KA)[:T].reshape(T * B, KA).double()
    gW0 = st.prior()[0].double()
    return gW0, A.t() @ X, A.abs().t() @ X.abs(), T * B + (dw_adds(T) if st.grads0 is not None else 0)


def check_all(st: LstmState, dw: bool = True) -> list:
    out = check_forward(st) + check_head(st) + check_backward(st)
    return out + check_dw(st) if dw else out


def check_inference(st: LstmState) -> list:
    """What ``forward`` / ``forward_windows`` leave: every forward step and pred (``st.x`` is the
    batch as packed, zero padding rows included). dy, the loss and the gradients are not its."""
    return check_forward(st) + [check_pred(st)]


def violations(checks) -> list:
    """[(name, t, *index, ratio)] of every recorded violation."""
    out = []
    for c in checks:
        for w, r in zip(c.where(), c.ratio.tolist()):
            out.append((c.name, *w, r))
    return out


def describe(checks) -> str:
    """The distribution of the violations: per tensor the count, the steps, the row / unit /
    gate ranges and the worst ratios."""
    lines = []
    for c in checks:
        if c.count == 0:
            continue
        ix = c.idx
        span = ["%d..%d" % (int(ix[:, d].min()), int(ix[:, d].max())) for d in range(ix.shape[1])]
        lines.append(f"{c.name}[t={c.t}]: {c.count} violations, index ranges {span} (first {KEEP}), "
                     f"worst ratio {c.worst:.3g}, first {c.where()[:4]} ratios {[round(r, 3) for r in c.ratio.tolist()[:4]]}")
    return "\n".join(lines)


def summary(checks) -> dict:
    """Per tensor: the worst ratio and the median slack share over all its steps."""
    out = {}
    for c in checks:
        w, s, n = out.get(c.name, (0.0, 0.0, 0))
        out[c.name] = (max(w, c.worst), s + c.share, n + 1)
    return {k: {"worst": round(w, 4), "share": round(s / n, 4)} for k, (w, s, n) in out.items()}
