"""The LSTM pack kernels, bit for bit: they move data and round once, so ``torch.equal`` against
host index formulas (wellflow/train/lstm_ref.py) is the assertion. ``Tensor.to(bfloat16)`` is
the round-to-nearest-even reference; the inputs hold values no bf16 represents, ties included."""
import pytest
import torch

from wellflow.train import lstm_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
H = 128


def _lib():
    from wellflow.ops.native import lib

    return lib()


def _values(shape, seed):
    """Generic fp32 values plus exact ties between two bf16 neighbours (to even: down and up), values
    a hair off a tie, large and tiny magnitudes, both signs."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g)
    flat = x.view(-1)
    sp = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), 1 + 2.0 ** -8 + 2.0 ** -23,
                       1 + 2.0 ** -8 - 2.0 ** -23, 3.0e38, -3.0e38, 1.0e-30, 255.5, 256.5 * 2, 0.0, -0.0,
                       0.1, 1 / 3, 65504.0, 1 - 2.0 ** -9, 1 - 2.0 ** -10])
    n = min(flat.numel() // 2, sp.numel() * 8)
    pos = torch.randperm(flat.numel(), generator=g)[:n]
    flat[pos] = sp.repeat(8)[:n]
    assert not torch.equal(x.to(BF).float(), x)
    return x


@pytest.mark.parametrize("F", [7, 9, 16, 63, 100, 127])
@pytest.mark.parametrize("B", [40, 64])
def test_pack_x_full_then_partial(F, B):
    C = _lib()
    T = 3
    KX = (F + 1 + 63) // 64 * 64
    KA = KX + H
    SENT, SENT2 = 3.0, -5.0
    XH = torch.full(((T + 1) * B * KA,), SENT, dtype=BF, device=DEV)
    x1 = _values((B, T, F), 1).to(DEV)
    C.lstm_pack_x(x1, XH, B, T, F, KX, H, True)
    torch.cuda.synchronize()
    v = XH.view(T + 1, B, KA)
    assert torch.equal(v[:T, :, :KX], R.pack_x_ref(x1, KX))                 # features RNE, the 1 column, zeros
    assert bool((v[:T, :, KX:] == SENT).all()) and bool((v[T] == SENT).all())  # h blocks and slab T untouched
    # partial pack over the previous contents: the chunks holding features and the 1 column (rounded
    # up to whole 64-B segments, csrc/lstm.hip launch_lstm_pack_x) change, the constant chunks stay
    cpr = min(KX // 8, ((F + 1 + 7) // 8 + 3) // 4 * 4)
    v[:T, :, cpr * 8:KX] = SENT2
    x2 = _values((B, T, F), 2).to(DEV)
    C.lstm_pack_x(x2, XH, B, T, F, KX, H, False)
    torch.cuda.synchronize()
    ref2 = R.pack_x_ref(x2, KX)
    assert torch.equal(v[:T, :, :cpr * 8], ref2[:, :, :cpr * 8])
    assert bool((v[:T, :, cpr * 8:KX] == SENT2).all())
    assert bool((v[:T, :, KX:] == SENT).all()) and bool((v[T] == SENT).all())
    if cpr * 8 < KX:
        assert not torch.equal(v[:T, :, :KX], ref2)  # the sentinel really sits in constant columns


def test_pack_x_refuses_an_unaligned_view():
    """The kernel's scalar branch for a base pointer off 16 B cannot be reached: the binding
    refuses the view (check_t), so the vector loads never see one."""
    C = _lib()
    B, T, F, KX = 40, 2, 16, 64
    XH = torch.zeros((T + 1) * B * (KX + H), dtype=BF, device=DEV)
    buf = torch.randn(B * T * F + 1, device=DEV)
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        C.lstm_pack_x(buf[1:].view(B, T, F), XH, B, T, F, KX, H, True)
    torch.cuda.synchronize()
    assert XH.abs().max().item() == 0.0


def _windows(table, starts, idx, T):
    """[B][T][F]: batch row b = table rows r0 .. r0 + T - 1, the id clamped to a valid window and
    the start to a valid row (csrc/lstm.hip lstm_pack_x_kernel)."""
    nrows, nwin = table.shape[0], starts.numel()
    r0 = starts[idx.clamp(0, nwin - 1)].clamp(0, nrows - T)
    return table.cpu()[r0[:, None] + torch.arange(T)[None, :]].to(DEV)


@pytest.mark.parametrize("F", [7, 9, 16, 63, 100, 127])
@pytest.mark.parametrize("B", [40, 64])
def test_pack_x_win_full_then_partial(F, B):
    """Windows read in place from the row table, the full pack and then the partial one over the
    previous contents (the route every training step after the first takes); ids and starts out
    of range are clamped to a valid window / row, never read out of the table."""
    C = _lib()
    T, nrows, nwin = 3, 57, 11
    KX = (F + 1 + 63) // 64 * 64
    KA = KX + H
    SENT, SENT2 = 3.0, -5.0
    g = torch.Generator().manual_seed(4)

    def ids():
        starts = torch.randint(0, nrows - T + 1, (nwin,), generator=g)
        starts[2], starts[5], starts[7] = -3, nrows - 1, nrows + 40  # clamped into [0, nrows - T]
        idx = torch.randint(0, nwin, (B,), generator=g)
        idx[0], idx[1], idx[2], idx[3], idx[4], idx[5] = -1, nwin, nwin + 1000, 2, 5, 7
        return starts, idx[torch.randperm(B, generator=g)]

    table1, (starts1, idx1) = _values((nrows, F), 3).to(DEV), ids()
    XH = torch.full(((T + 1) * B * KA,), SENT, dtype=BF, device=DEV)
    C.lstm_pack_x_win(table1, starts1.to(DEV), idx1.to(DEV), XH, B, T, F, KX, H, True)
    torch.cuda.synchronize()
    v = XH.view(T + 1, B, KA)
    assert torch.equal(v[:T, :, :KX], R.pack_x_ref(_windows(table1, starts1, idx1, T), KX))
    assert bool((v[:T, :, KX:] == SENT).all()) and bool((v[T] == SENT).all())
    # partial pack of other windows of another table: the feature chunks change, the constant ones stay
    cpr = min(KX // 8, ((F + 1 + 7) // 8 + 3) // 4 * 4)
    v[:T, :, cpr * 8:KX] = SENT2
    table2, (starts2, idx2) = _values((nrows, F), 8).to(DEV), ids()
    C.lstm_pack_x_win(table2, starts2.to(DEV), idx2.to(DEV), XH, B, T, F, KX, H, False)
    torch.cuda.synchronize()
    ref2 = R.pack_x_ref(_windows(table2, starts2, idx2, T), KX)
    assert torch.equal(v[:T, :, :cpr * 8], ref2[:, :, :cpr * 8])
    assert not torch.equal(ref2, R.pack_x_ref(_windows(table1, starts1, idx1, T), KX))
    assert bool((v[:T, :, cpr * 8:KX] == SENT2).all())
    assert bool((v[:T, :, KX:] == SENT).all()) and bool((v[T] == SENT).all())


def _weight_images(W, KX):
    """Wp = bf16(W * scale) in gate_col row order, WhhT = bf16(W_hh)^T in dg_col column order."""
    G, KA = W.shape
    sig = torch.tensor(-1.4426950408889634, dtype=torch.float32, device=W.device)  # csrc/common.h
    tnh = torch.tensor(2.8853900817779268, dtype=torch.float32, device=W.device)
    scale = torch.stack([sig, sig, tnh, sig])
    Wp = torch.zeros(G, KA, dtype=BF, device=W.device)
    Wp[R.gate_col_index(G // 4, W.device)] = (R.decode_w_rows(W, G // 4) * scale[None, :, None]).to(BF)
    return Wp.view(-1), W[:, KX:].to(BF).t().contiguous().view(-1)


@pytest.mark.parametrize("F", [16, 100])  # KX = 64, 128
def test_pack_weights_and_adam_pack_images(F):
    from wellflow.models.lstm import NativeLSTM
    from wellflow.optim.flat import FlatAdam

    eng = NativeLSTM(F, H, 2, 32, device=DEV)
    KX = eng.lay.KX
    assert KX == (64 if F == 16 else 128)
    eng.params.copy_(_values(eng.params.shape, 5).to(DEV) * 0.1)
    eng.sync_weights()
    torch.cuda.synchronize()
    W, _, _ = eng.lay.views(eng.params)
    Wp, WhhT = _weight_images(W, KX)
    assert torch.equal(eng.Wp, Wp) and torch.equal(eng.WhhT, WhhT)
    # the fused Adam launch writes the images of the parameters it stores
    opt = FlatAdam(eng.params, eng.grads, lr=1e-2, zero_grads=True, writeback=eng)
    assert eng.fused_adam_ok(opt)
    eng.grads.copy_(torch.randn(eng.grads.shape, generator=torch.Generator().manual_seed(6)).to(DEV))
    before = eng.params.clone()
    opt.step()
    torch.cuda.synchronize()
    assert not torch.equal(before, eng.params)
    Wp, WhhT = _weight_images(eng.lay.views(eng.params)[0], KX)
    assert torch.equal(eng.Wp, Wp) and torch.equal(eng.WhhT, WhhT)
