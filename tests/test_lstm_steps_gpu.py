"""Every LSTM kernel path against float64, one step at a time (wellflow/train/lstm_ref.py).

Each case runs ``forward_backward`` twice on one engine with different data (the second call
goes through the partial x pack and re-uses Cst slab 0, the sync buffers and dcarry), copies
the state out after each call and checks every step from the device's own inputs to it:
``|dev - ref| <= half a bf16 ulp of ref + slack`` at every element of S, Cst, h and DG, the
head and the weight gradient within their dot-product bounds. The path each case is meant to
take is asserted, not assumed: the persistent flags, ``persistent_error() == 0`` and, from the
STAT block's launch and workgroup totals, the (sub-batches, units per workgroup) instantiation
that ``persistent_split`` picks (mirrored in tests/lstm_plans.py), which pins the NC / NRT variant.

tests/test_lstm_steps_cpu.py proves the checker: an fp32 emulation passes under the caps and
its mutations of the state are each rejected where they were made.
"""
import json

import pytest
import torch

from wellflow.train import lstm_ref as R

from lstm_plans import _cus, bwd_plan, dw_uses_slab, fwd_plan

pytestmark = pytest.mark.gpu

DEV = "cuda"


# the launchers' rules (which persistent instantiation, which dW route): tests/lstm_plans.py
def smallest_batch(pred, step):
    for B in range(step, 1 << 17, step):
        if pred(B):
            return B
    raise AssertionError("no batch selects this variant on this device")


# ------------------------------------------------------------------ one case
def run_case(B, H, T, F, *, persistent=True, persistent_bwd=True, variants=(6, 8), loss="mse", ksplit=0,
             slab="default", chunk=0, dw=True, want_fwd=None, want_bwd=None, clip=6.0):
    from wellflow.data.synth import synth_lstm_batch
    from wellflow.models.lstm import NativeLSTM, init_lstm_flat

    eng = NativeLSTM(F, H, T, B, device=DEV, loss=loss, clip=clip)
    eng.persistent, eng.persistent_bwd = persistent, persistent_bwd
    eng.fwd_variant, eng.bwd_variant = variants
    eng.dw_ksplit, eng.dw_chunk = ksplit, chunk
    if slab is None:
        eng.dw_slab = None
    elif slab != "default":
        eng.dw_slab = torch.empty(slab * eng.lay.G * eng.lay.KA, dtype=torch.float32, device=DEV)
    eng.params.copy_(init_lstm_flat(F, H, seed=0).to(DEV))
    eng.sync_weights()
    fp = fwd_plan(B, H, F) if persistent else None
    bp = bwd_plan(B, H) if persistent_bwd and chunk <= 0 and T >= 2 else None
    if want_fwd is not None:
        assert (fp is not None) == want_fwd, (fp, want_fwd)
    if want_bwd is not None:
        assert (bp is not None) == want_bwd, (bp, want_bwd)
    stats = {}
    for call, seed in enumerate((0, 1)):
        x, y = synth_lstm_batch(B, T, F, seed=seed)
        x, y = x.float().to(DEV), y.float().to(DEV)
        if loss == "mae_clip" and call == 1:
            # the clip boundary, exactly: y - pred == clip at row 0, 0 at row 1, past it at row 2
            # (row 0 swapped for the first row whose pred + clip is an fp32 number)
            p = eng.forward(x).clone()
            b0 = int((((p + clip) - p) == clip).nonzero()[0])
            x[[0, b0]] = x[[b0, 0]]
            p[[0, b0]] = p[[b0, 0]]
            y[0], y[1], y[2] = p[0] + clip, p[1], p[2] - 2 * clip
            assert (y[0] - p[0]).item() == clip
        eng.forward_backward(x, y, grad_scale=1.0 / B)
        torch.cuda.synchronize()
        assert eng.last_forward_persistent == (fp is not None), "forward took the other path"
        assert eng.last_backward_persistent == (bp is not None or (persistent_bwd and chunk <= 0 and T < 2))
        assert eng.persistent_error() == 0, eng.persistent_stats()
        st = R.LstmState.of_engine(eng, x, y, 1.0 / B)
        if loss == "mae_clip" and call == 1:
            gs32 = torch.tensor(1.0 / B, dtype=torch.float32).item()
            assert (st.y[0] - st.pred[0]).item() == clip and st.dy[0].item() == -gs32  # on the boundary: inside
            assert st.dy[1].item() == 0.0 and st.dy[2].item() == 0.0
        checks = R.check_all(st, dw=dw)
        assert not R.violations(checks), f"call {call}:\n" + R.describe(checks)
        stats[call] = R.summary(checks)
    ps = eng.persistent_stats()
    nf = 2 + (1 if loss == "mae_clip" else 0)  # forward launches: the boundary probe is one more
    if fp is not None:
        assert ps["forward"]["launches"] == nf * fp[0] and ps["forward"]["expect_wg"] == nf * fp[0] * fp[2], (ps, fp)
    if bp is not None:
        assert ps["backward"]["launches"] == 2 * bp[0] and ps["backward"]["expect_wg"] == 2 * bp[0] * bp[2], (ps, bp)
    print("LSTMSTEPS " + json.dumps({"case": [B, H, T, F], "fwd": fp, "bwd": bp, "variants": list(variants),
                                      "loss": loss, "stats": stats[1]}))
    return fp, bp


def test_checker_rejects_a_touched_device_state():
    """The checker's teeth on the device's own state (the nine mutations proper run on the CPU
    emulation): one saved gate, one h and one gate gradient of a correct run, each moved by two
    bf16 ulps, are each reported where they were moved."""
    from wellflow.data.synth import synth_lstm_batch
    from wellflow.models.lstm import NativeLSTM, init_lstm_flat

    B, H, T, F = 64, 128, 3, 16
    eng = NativeLSTM(F, H, T, B, device=DEV)
    eng.params.copy_(init_lstm_flat(F, H, seed=0).to(DEV))
    eng.sync_weights()
    x, y = synth_lstm_batch(B, T, F, seed=0)
    x, y = x.float().to(DEV), y.float().to(DEV)
    eng.forward_backward(x, y, grad_scale=1.0 / B)
    torch.cuda.synchronize()
    st = R.LstmState.of_engine(eng, x, y, 1.0 / B)
    assert not R.violations(R.check_all(st))

    def bump(flat, off):  # two bf16 numbers further from zero
        flat.view(torch.int16)[off] += 2

    t, m, u, g = 1, 37, 101, 2
    bump(st.S, t * R.fn_rows(B) * 4 * H + int(R.s_index(B, H)[m, u, g]))
    v = R.violations(R.check_forward(st))
    assert [w[:5] for w in v] == [("S", t, m, u, g)], v
    st = R.LstmState.of_engine(eng, x, y, 1.0 / B)
    bump(st.XH, ((T * B) + m) * st.KA + st.KX + u)  # h_T: the head reads it
    v = R.violations(R.check_forward(st) + R.check_head(st))
    assert ("h", T - 1, m, u) in [w[:4] for w in v] and all(w[0] in ("h", "pred", "gw_out") for w in v), v
    st = R.LstmState.of_engine(eng, x, y, 1.0 / B)
    bump(st.DG, (t * B + m) * 4 * H + 4 * u + g)
    v = R.violations(R.check_backward(st))
    assert ("DG", t, m, u, g) in [w[:5] for w in v] and all(w[1] <= t for w in v), v


# ------------------------------------------------------------------ per-step kernels
@pytest.mark.parametrize("B,H,T,F", [(40, 128, 4, 9), (96, 256, 3, 16), (144, 512, 2, 100)])
def test_per_step_register_staged(B, H, T, F):
    """Variants 0 / 0, any batch: row guards, FN padding rows (B = 40), the scalar x pack."""
    run_case(B, H, T, F, persistent=False, persistent_bwd=False, variants=(0, 0))


@pytest.mark.parametrize("B,H,T,F", [(256, 128, 3, 16), (256, 256, 3, 64), (256, 512, 3, 16)])
def test_per_step_direct_to_lds_rings(B, H, T, F):
    """Variants 6 / 8. The ring tiles fall back to the register-staged kernel silently when B is
    no multiple of their tile (256 rows forward, 128 backward; 256 gate columns): B = 256 is.
    No device observable tells the two kernels apart, so the launchers' precondition (csrc/lstm.hip
    fwd_cfg / bwd_cfg) is what is asserted."""
    assert B % 256 == 0 and B % 128 == 0 and (4 * H) % 256 == 0
    run_case(B, H, T, F, persistent=False, persistent_bwd=False, variants=(6, 8))


# ------------------------------------------------------------------ persistent forward
PF = [(KT, NC) for KT in (6, 10, 18, 8, 12) for NC in (1, 2, 4, 8)] + [(20, 1), (20, 8)]


@pytest.mark.parametrize("KT,NC", PF)
def test_persistent_forward_every_instantiation(KT, NC):
    """All 22 built (KT, NC) of csrc/lstm_persistent.hip: KT = KA / 32 (6, 10, 18: KX = 64 at
    H = 128, 256, 512; 8, 12, 20: KX = 128, F = 100). NC = 1 at B = 64; NC > 1 at the smallest
    batch whose split picks it (on 256 CUs at H = 512: 1088, 2176, 4352 — grids that are no
    power of two). The persistent backward runs too wherever B % 64 == 0."""
    H, F = {6: (128, 16), 10: (256, 16), 18: (512, 16), 8: (128, 100), 12: (256, 100), 20: (512, 100)}[KT]
    assert ((F + 1 + 63) // 64 * 64 + H) // 32 == KT
    if NC == 1:
        B = 64
    else:
        B = smallest_batch(lambda b: (fwd_plan(b, H, F) or (0, 0))[1] == NC, 32)
    T = 3 if NC == 1 else 2
    fp, bp = run_case(B, H, T, F, want_fwd=True)
    assert fp[1] == NC
    if B % 64 == 0:
        assert bp is not None


def test_persistent_forward_bench_variant():
    """(8192, 512): the benchmark's instantiation. Forward and DG checks (dW is covered at small K)."""
    fp, bp = run_case(8192, 512, 2, 16, dw=False, want_fwd=True, want_bwd=True)
    if _cus() == 256:
        assert fp == (1, 8, 256) and bp == (1, 4, 256)


def test_persistent_forward_two_sub_batches():
    """The smallest B at H = 128 that runs as two sub-batch launches (row_off != 0)."""
    B = smallest_batch(lambda b: (fwd_plan(b, 128, 16) or (0,))[0] == 2, 32)
    fp, _ = run_case(B, 128, 2, 16, dw=False, want_fwd=True)
    assert fp[0] == 2


def test_persistent_forward_single_chunk_backward_falls_back():
    """(32, 128): one 32-row chunk; B % 64 != 0, so the backward runs the per-step kernels."""
    run_case(32, 128, 3, 16, want_fwd=True, want_bwd=False)


# ------------------------------------------------------------------ persistent backward
@pytest.mark.parametrize("H", [128, 256, 512])
@pytest.mark.parametrize("units", [1, 2, 4])
def test_persistent_backward_every_units_variant(H, units):
    """The smallest B that selects each units-per-workgroup variant (NRT = 4, 8, 16 row tiles)
    of csrc/lstm_persistent_bwd.hip, T = 3: two persistent steps after step T-1."""
    B = smallest_batch(lambda b: (bwd_plan(b, H) or (0, 0))[1] == units, 64)
    _, bp = run_case(B, H, 3, 16, dw=False, want_bwd=True)
    assert bp[1] == units


# ------------------------------------------------------------------ dW routes
@pytest.mark.parametrize("H", [512, 128, 256])
@pytest.mark.parametrize("route", ["ksplit0", "ksplit3_slab", "atomics", "chunk2"])
def test_dw_routes(H, route):
    """(256, H, 3, 16): KA = 576 takes the 256x288 tile, 192 the 256x192, 320 the 256x128.
    ksplit 0 (one split); ksplit 3 with a three-split slab (the constructor's one-split slab
    would send three splits to atomics); no slab (atomics); dw_chunk = 2 at T = 5 (the
    side-stream route, per-step backward). Only the 256x288 tile has a slab route: at H = 128
    and 256 the ``ksplit3_slab`` case runs the same atomics as ``atomics``. No device observable
    tells the routes apart, so the launcher's own condition is mirrored (dw_uses_slab) and
    asserted on the engine as configured: the slab route at H = 512 / ksplit3_slab and nowhere else."""
    from wellflow.models.lstm import LstmLayout, NativeLSTM

    kw = {"ksplit0": dict(ksplit=0), "ksplit3_slab": dict(ksplit=3, slab=3), "atomics": dict(ksplit=3, slab=None),
          "chunk2": dict(chunk=2)}[route]
    B, T, lay = 256, 5 if route == "chunk2" else 3, LstmLayout(16, H)
    slab = {"default": NativeLSTM._dw_slab_splits(lay.G, lay.KA, T * B, DEV), None: None, 3: 3}[kw.get("slab", "default")]
    if route == "chunk2":
        slab = None  # forward_backward passes no slab to the chunked route
    ks = kw.get("ksplit", 0) or max(1, min(32, T * B // 16384))
    uses = dw_uses_slab(lay.G, lay.KA, T * B, ks, None if slab is None else slab * lay.G * lay.KA)
    assert uses == (H == 512 and route == "ksplit3_slab")
    if route == "ksplit3_slab":  # and the constructor's slab would not have held three splits
        assert not dw_uses_slab(lay.G, lay.KA, T * B, 3, NativeLSTM._dw_slab_splits(lay.G, lay.KA, T * B, DEV) * lay.G * lay.KA)
    run_case(B, H, T, 16, want_fwd=True, want_bwd=route != "chunk2", **kw)


# ------------------------------------------------------------------ loss
@pytest.mark.parametrize("B,H,T,F,per_step", [(40, 128, 4, 9, True), (256, 512, 3, 16, False), (1088, 512, 2, 16, False)])
def test_mae_clip_head(B, H, T, F, per_step):
    """head_fwd + loss + head_bwd_w (the mse cases above take the fused head where the shape
    allows): dy exact, the clip boundary included."""
    if per_step:
        run_case(B, H, T, F, persistent=False, persistent_bwd=False, variants=(0, 0), loss="mae_clip", clip=0.5)
    else:
        run_case(B, H, T, F, loss="mae_clip", clip=0.5)
