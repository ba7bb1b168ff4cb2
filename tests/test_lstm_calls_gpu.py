"""The LSTM engine through the calls training and scoring make, against float64, one step at a
time (wellflow/train/lstm_ref.py). tests/test_lstm_steps_gpu.py reaches every kernel path through
``forward_backward(x, y, gs)`` on a zeroed bucket; here the same paths are reached the way
train/step.py, Trainer.evaluate and scoring.py reach them:

* ``forward_backward(..., zero_grads=False, loss_into=acc)`` on a bucket that already holds a
  gradient: every dW route and both heads must ADD to it (``grads0`` / ``loss0`` of the checker);
* ``rows=``: the batch read in place from a window table, the targets ``index_select``ed;
* ``forward`` on a short batch and ``forward_windows`` with scoring's padded ids, on an engine a
  training call has just left dirty, touching no training state;
* the production step captured in a graph and replayed with new rows.

Every tolerance is the checker's derived bound or exact equality; the prior is the lattice of
tests/lstm_plans.py, whose teeth tests/test_lstm_steps_cpu.py asserts. The path each case takes
is asserted as in test_lstm_steps_gpu.py (persistent flags, ``persistent_error() == 0``, STAT
totals). Each case prints one ``LSTMCALLS {json}`` line: the worst error / bound ratio per check.
"""
import json

import pytest
import torch

from wellflow.train import lstm_ref as R

import lstm_plans as P
from lstm_plans import bwd_plan, dw_uses_slab, fwd_plan

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


def same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def synth(B, T, F, seed):
    from wellflow.data.synth import synth_lstm_batch

    x, y = synth_lstm_batch(B, T, F, seed=seed)
    return x.float().to(DEV), y.float().to(DEV)


def windows(B, T, F, seed=0):
    """(SeriesWindows on the device, yall, [ids0, ids1, ids2], host gather of a batch)."""
    from wellflow.data.features import SeriesWindows

    table, starts, yall, ids = P.window_rows(B, T, F, seed)
    win = SeriesWindows(table.to(DEV), starts.to(DEV), T)
    return win, yall.to(DEV), [i.to(DEV) for i in ids], lambda i: P.gather_windows(table, starts, i, T).to(DEV)


class Case:
    """One engine, configured like test_lstm_steps_gpu.run_case, and the calls made on it: each
    asserts the path it took, snapshots the state and runs the checker; ``finish`` compares the
    STAT totals with the number of passes made."""

    def __init__(self, B, H, T, F, *, persistent=True, persistent_bwd=True, variants=(6, 8), loss="mse", ksplit=0,
                 slab="default", chunk=0, want_fwd=None, want_bwd=None, clip=6.0):
        from wellflow.models.lstm import NativeLSTM, init_lstm_flat

        self.dims = (B, H, T, F)
        eng = self.eng = NativeLSTM(F, H, T, B, device=DEV, loss=loss, clip=clip)
        eng.persistent, eng.persistent_bwd = persistent, persistent_bwd
        eng.fwd_variant, eng.bwd_variant = variants
        eng.dw_ksplit, eng.dw_chunk = ksplit, chunk
        if slab is None:
            eng.dw_slab = None
        elif slab != "default":
            eng.dw_slab = torch.empty(slab * eng.lay.G * eng.lay.KA, dtype=torch.float32, device=DEV)
        eng.params.copy_(init_lstm_flat(F, H, seed=0).to(DEV))
        eng.sync_weights()
        self.fp = fwd_plan(B, H, F) if persistent else None
        self.bp = bwd_plan(B, H) if persistent_bwd and chunk <= 0 and T >= 2 else None
        self.want_bwd_flag = self.bp is not None or (persistent_bwd and chunk <= 0 and T < 2)
        if want_fwd is not None:
            assert (self.fp is not None) == want_fwd, (self.fp, want_fwd)
        if want_bwd is not None:
            assert (self.bp is not None) == want_bwd, (self.bp, want_bwd)
        self.gs = 1.0 / B
        self.acc = torch.full((1,), P.LOSS0, dtype=torch.float32, device=DEV)  # the caller's loss accumulator
        self.sentinel = -7.25
        eng.loss_sum.fill_(self.sentinel)  # the engine's own: no call here may touch it
        self.nf = self.nb = 0
        self.worst = {}

    def _record(self, checks, what):
        assert not R.violations(checks), f"{what}:\n" + R.describe(checks)
        for k, v in R.summary(checks).items():
            self.worst[k] = max(self.worst.get(k, 0.0), v["worst"])

    def _after(self, backward):
        eng = self.eng
        torch.cuda.synchronize()
        self.nf += 1
        assert eng.last_forward_persistent == (self.fp is not None), "forward took the other path"
        if backward:
            self.nb += 1
            assert eng.last_backward_persistent == self.want_bwd_flag, "backward took the other path"
        assert eng.persistent_error() == 0, eng.persistent_stats()
        assert eng.loss_sum.item() == self.sentinel

    def train(self, x, y, *, rows=None, dense=None, what="train", zero_prior=False):
        """forward_backward(x, y, gs, zero_grads=False, loss_into=acc[, rows=]) on the bucket as it
        stands. ``dense`` = (x [B][T][F], y [B]) of the batch when it is read through ``rows``.
        ``zero_prior``: the bucket is exactly zero (asserted) and the checker gets no prior: the
        bound of a zeroed bucket."""
        eng = self.eng
        g0, l0 = eng.grads.clone(), self.acc.clone()
        if zero_prior:
            assert not bool(g0.any())
        out = eng.forward_backward(x, y, self.gs, zero_grads=False, loss_into=self.acc, rows=rows)
        assert out is self.acc
        self._after(True)
        xd, yd = (x, y) if rows is None else dense
        st = R.LstmState.of_engine(eng, xd, yd, self.gs, grads0=None if zero_prior else g0, loss0=l0, loss_acc=self.acc)
        self._record(R.check_all(st), what)
        return st

    def infer(self, pred, x_packed, what):
        """After a forward / forward_windows that returned ``pred``: x_packed is the [B][T][F] batch
        as the engine must have packed it."""
        self._after(False)
        st = R.LstmState.of_engine(self.eng, x_packed, torch.zeros(self.dims[0], device=DEV), self.gs)
        self._record(R.check_inference(st), what)
        assert pred.data_ptr() == self.eng.pred.data_ptr()
        return st

    def finish(self, name, **extra):
        ps = self.eng.persistent_stats()
        fp, bp = self.fp, self.bp
        if fp is not None:
            assert ps["forward"]["launches"] == self.nf * fp[0] and ps["forward"]["expect_wg"] == self.nf * fp[0] * fp[2], (ps, fp)
        if bp is not None:
            assert ps["backward"]["launches"] == self.nb * bp[0] and ps["backward"]["expect_wg"] == self.nb * bp[0] * bp[2], (ps, bp)
        assert max(self.worst.values()) <= 1.0
        print("LSTMCALLS " + json.dumps({"test": name, "case": list(self.dims), "fwd": fp, "bwd": bp,
                                          "loss": self.eng.loss_kind, "worst": self.worst, **extra}))


# ------------------------------------------------------------------ a bucket that holds a gradient
ROUTES = {"ksplit0": dict(ksplit=0), "ksplit3_slab": dict(ksplit=3, slab=3), "atomics": dict(ksplit=3, slab=None),
          "chunk2": dict(chunk=2)}
ACCUMULATE = ([(256, H, 5 if r == "chunk2" else 3, 16, r, "mse") for H in (128, 256, 512) for r in ROUTES]
              + [(64, 256, 3, 100, "ksplit0", "mse"), (64, 512, 3, 100, "ksplit0", "mse"),
                 (40, 128, 4, 9, "per_step", "mse"), (40, 128, 4, 9, "per_step", "mae_clip"),
                 (256, 512, 3, 16, "ksplit0", "mae_clip")])


@pytest.mark.parametrize("B,H,T,F,route,loss", ACCUMULATE)
def test_accumulates_into_a_prior_bucket(B, H, T, F, route, loss):
    """Two accumulating calls on one engine: the first on the lattice prior (nonzero at every word
    of the bucket, gW's padding columns included) with the accumulator preset to 3.0, the second on
    what the first left. gW (split-K atomics, the one-split atomic epilogue, the slab and its
    reduce, side-stream chunks; the 256x288, 256x192 and 256x128 tiles at KA = 576, 192, 320 and
    the generic tiles at KA = 384 / 640 and B = 40), gw_out, gb_out and the loss must each equal
    prior + sum within the bound; gW's padding columns must still hold the prior, bit for bit
    (``gW_pad``). mae_clip takes head_fwd + loss_kernel + head_bwd_w, mse the fused head."""
    from wellflow.models.lstm import LstmLayout, NativeLSTM

    lay = LstmLayout(F, H)
    if route == "per_step":
        c = Case(B, H, T, F, persistent=False, persistent_bwd=False, variants=(0, 0), loss=loss)
    else:
        kw = ROUTES[route]
        # the launcher's own slab condition, as in test_lstm_steps_gpu.test_dw_routes: the slab
        # route at H = 512 / ksplit3_slab and nowhere else
        slab = {"default": NativeLSTM._dw_slab_splits(lay.G, lay.KA, T * B, DEV), None: None, 3: 3}[kw.get("slab", "default")]
        if route == "chunk2":
            slab = None
        ks = kw.get("ksplit", 0) or max(1, min(32, T * B // 16384))
        uses = dw_uses_slab(lay.G, lay.KA, T * B, ks, None if slab is None else slab * lay.G * lay.KA)
        assert uses == (H == 512 and F == 16 and route == "ksplit3_slab")
        c = Case(B, H, T, F, loss=loss, want_fwd=True, want_bwd=route != "chunk2", **kw)
    assert lay.KA == {(128, 16): 192, (256, 16): 320, (512, 16): 576, (256, 100): 384, (512, 100): 640, (128, 9): 192}[(H, F)]
    c.eng.grads.copy_(P.lattice_prior(lay, device=DEV))
    prior = c.eng.grads.clone()
    assert bool((prior != 0).all())
    for call in (0, 1):
        st = c.train(*synth(B, T, F, seed=call), what=f"call {call}")
        assert same_bits(st.grads0, prior)  # what the checker was given is what the bucket held
        pad = st.views(st.grads)[0][:, F + 1:st.KX]
        assert same_bits(pad.contiguous(), st.views(P.lattice_prior(lay, device=DEV))[0][:, F + 1:st.KX].contiguous())
        assert st.loss_sum.item() > st.loss0.item() >= P.LOSS0
        prior = c.eng.grads.clone()
    c.finish("accumulate", route=route)


# ------------------------------------------------------------------ the production step
@pytest.mark.parametrize("B,H,T,F", [(64, 128, 3, 16), (256, 512, 3, 16)])
def test_zero_prior_is_the_production_step(B, H, T, F):
    """train/step.py's step, three times: the row-indexed accumulating call on a bucket the fused
    Adam launch cleared, then that launch. After each update the WHOLE bucket is exactly zero and
    Wp / WhhT are the host encodings of the new parameters; the accumulator holds the three loss
    sums within the sum of the three per-call bounds."""
    from test_lstm_pack_gpu import _weight_images
    from wellflow.optim.flat import FlatAdam

    c = Case(B, H, T, F, want_fwd=True, want_bwd=True)
    eng = c.eng
    opt = FlatAdam(eng.params, eng.grads, lr=1e-3, zero_grads=True, writeback=eng)
    assert eng.fused_adam_ok(opt)
    win, yall, ids, gather = windows(B, T, F)
    c.acc.zero_()
    total = 0.0
    for k in range(3):
        st = c.train(win, yall, rows=ids[k], dense=(gather(ids[k]), yall[ids[k]]), what=f"step {k}", zero_prior=True)
        total += float(R.head_terms(st)["loss_sum"][1])
        before = eng.params.clone()
        opt.step()
        torch.cuda.synchronize()
        assert not bool(eng.grads.any()), "the update left words of the bucket uncleared"
        assert not torch.equal(before, eng.params)
        Wp, WhhT = _weight_images(eng.lay.views(eng.params)[0], eng.lay.KX)
        assert same_bits(eng.Wp, Wp) and same_bits(eng.WhhT, WhhT)
    # each call's bound is (B + 4 + adds) u (acc before + its sum) <= (B + 4 + adds) u total
    bound = 3 * (B + 4 + R.head_adds(B)[0]) * R.U32 * total
    err = abs(c.acc.double().item() - total)
    assert err <= bound, (err, bound)
    c.finish("production_step", acc_ratio=round(err / bound, 4))


# ------------------------------------------------------------------ windows read in place
@pytest.mark.parametrize("F", [9, 16, 100])
@pytest.mark.parametrize("B,per_step", [(64, False), (40, True)])
def test_window_rows_step(B, per_step, F):
    """rows= on a fresh engine (the window pack writes XH's constant columns), then a dense batch
    (the plain pack's partial route trusts them), then rows= again: overlapping windows, a shuffled
    subset of ids with two of them twice. The reference batch is gathered on the host; ``xblock``
    is exact, and the bucket keeps accumulating over the three calls."""
    H, T = 128, 4
    kw = dict(persistent=False, persistent_bwd=False, variants=(0, 0)) if per_step else dict(want_fwd=True, want_bwd=True)
    c = Case(B, H, T, F, **kw)
    win, yall, ids, gather = windows(B, T, F)
    assert win.rows.shape[0] == 3 * B + T and ids[0].unique().numel() == B - 2
    assert not c.eng._xh_const
    c.train(win, yall, rows=ids[0], dense=(gather(ids[0]), yall[ids[0]]), what="rows 0")
    assert c.eng._xh_const
    c.train(*synth(B, T, F, seed=1), what="dense")
    c.train(win, yall, rows=ids[2], dense=(gather(ids[2]), yall[ids[2]]), what="rows 2")
    assert c.worst["xblock"] == 0.0
    c.finish("window_rows")


# ------------------------------------------------------------------ inference on a dirty engine
@pytest.mark.parametrize("B,H,T,F,per_step", [(64, 128, 4, 16, False), (40, 128, 4, 16, True), (256, 512, 3, 16, False)])
def test_inference_after_training(B, H, T, F, per_step):
    """Trainer.evaluate / scoring after a training call left XH, Cst, S and dcarry dirty:
    ``forward`` on 1, B - 1 and B rows (zero padding rows), ``forward_windows`` with scoring's
    padded id vector. Every forward step and pred within the bounds against the padded batch;
    grads, DG, dy, the engine's loss_sum and the caller's accumulator bit-identical to before;
    and a training call afterwards passes every check."""
    kw = dict(persistent=False, persistent_bwd=False, variants=(0, 0)) if per_step else dict(want_fwd=True, want_bwd=True)
    c = Case(B, H, T, F, **kw)
    eng = c.eng
    c.train(*synth(B, T, F, seed=0), what="train 0")
    snap = [t.clone() for t in (eng.grads, eng.DG, eng.dy, eng.loss_sum, c.acc)]

    def untouched():
        return all(same_bits(a, b) for a, b in zip(snap, (eng.grads, eng.DG, eng.dy, eng.loss_sum, c.acc)))

    x, _ = synth(B, T, F, seed=1)
    const = torch.zeros(eng.lay.KX, dtype=torch.bfloat16, device=DEV)  # a padding row: [0 ... | 1 | 0 ...]
    const[F] = 1.0
    for b in (1, B - 1, B):
        pred = eng.forward(x[:b])
        xp = torch.zeros_like(x)
        xp[:b] = x[:b]
        st = c.infer(pred, xp, f"forward {b}")
        assert pred.shape == (b,)
        if b < B:
            blk = st.XH.view(T + 1, B, st.KA)[:T, b:, :st.KX]
            assert same_bits(blk.contiguous(), const.expand_as(blk).contiguous())
        assert untouched(), f"forward({b}) touched training state"
    win, yall, _, gather = windows(B, T, F)
    W = len(win)
    a = W - 5
    ids = torch.arange(a, a + B, device=DEV).clamp_(max=W - 1)  # scoring.py LstmPass.forward: the last id repeated
    pred = eng.forward_windows(win, ids)
    c.infer(pred, gather(ids), "forward_windows")
    assert pred.shape == (B,)
    assert untouched(), "forward_windows touched training state"
    c.train(*synth(B, T, F, seed=2), what="train 2")
    c.finish("inference_after_training")


# ------------------------------------------------------------------ the captured step
def test_captured_step_replays_with_new_rows():
    """The production call captured in a graph (the recipe of test_determinism_gpu.py: eager
    warm-up on a side stream, engine defaults) and replayed twice, each time with new ids copied
    into the captured buffer and the bucket zeroed by hand."""
    B, H, T, F = 64, 128, 3, 16
    c = Case(B, H, T, F, want_fwd=True, want_bwd=True)
    eng = c.eng
    win, yall, ids, gather = windows(B, T, F)
    buf = ids[0].clone()

    def body():
        eng.forward_backward(win, yall, c.gs, zero_grads=False, loss_into=c.acc, rows=buf)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            body()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    c.nf, c.nb = 2, 2
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        body()
    for k in (1, 2):
        buf.copy_(ids[k])
        eng.grads.zero_()
        l0 = c.acc.clone()
        g.replay()
        c._after(True)
        st = R.LstmState.of_engine(eng, gather(ids[k]), yall[ids[k]], c.gs, loss0=l0, loss_acc=c.acc)
        c._record(R.check_all(st), f"replay {k}")
    c.finish("captured_step")


# ------------------------------------------------------------------ the checker on device state
def test_checker_rejects_a_dropped_prior_on_device_state():
    """The prior's teeth on the device's own state (the mutations proper run on the CPU emulation):
    on a correct accumulating run's snapshot the prior is subtracted from one gW element, from
    gb_out and from the accumulator; each is reported where it was made."""
    from wellflow.models.lstm import LstmLayout

    B, H, T, F = 64, 128, 3, 16
    lay = LstmLayout(F, H)
    c = Case(B, H, T, F)
    c.eng.grads.copy_(P.lattice_prior(lay, device=DEV))
    st = c.train(*synth(B, T, F, seed=0))
    r, col = 301, 100
    gW, _, gb_out = st.views(st.grads)
    p, good = st.prior(), st.grads.clone()
    gW[r, col] -= p[0][r, col]
    v = R.violations(R.check_all(st))
    assert [w[:4] for w in v] == [("gW", -1, r, col)], v
    st.grads.copy_(good)
    gb_out -= p[2]
    v = R.violations(R.check_all(st))
    assert [w[:3] for w in v] == [("gb_out", -1, 0)], v
    st.grads.copy_(good)
    st.loss_sum -= p[3]
    v = R.violations(R.check_all(st))
    assert [w[:3] for w in v] == [("loss_sum", -1, 0)], v
