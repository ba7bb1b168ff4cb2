"""Shared by tests/test_lstm_steps_gpu.py, tests/test_lstm_calls_gpu.py and tests/test_lstm_steps_cpu.py:
host mirrors of the LSTM launchers' rules (which persistent instantiation, which dW route a shape
takes), and the inputs of the accumulating / row-indexed calls (the lattice prior, a window table).
Nothing here is reference arithmetic: that is wellflow/train/lstm_ref.py."""
import torch


# ------------------------------------------------------------------ the launchers' rules
def persistent_split(B, row_quantum, max_units, cols, cus, unit_mask):
    """csrc/lstm_persistent.hip persistent_split: the fewest equal sub-batches, then the fewest
    units per workgroup, whose grid fits one workgroup per CU. -> (nsub, units) or None."""
    for nsub in range(1, 65):
        if B % nsub or (B // nsub) % row_quantum:
            continue
        Bs = B // nsub
        u = 1
        while u <= max_units:
            if (unit_mask >> (u.bit_length() - 1)) & 1 and Bs % (row_quantum * u) == 0 \
                    and Bs // (row_quantum * u) * cols <= cus:
                return nsub, u
            u *= 2
    return None


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def fwd_plan(B, H, F):
    """launch_lstm_fwd_persistent: (nsub, NC, grid) or None (per-step kernels)."""
    KX = (F + 1 + 63) // 64 * 64
    KA = KX + H
    if B % 32 or KX not in (64, 128) or H not in (128, 256, 512) or B * KA * 2 >= 2 ** 31 - 1:
        return None
    NB = 4 * H // 256
    p = persistent_split(B, 32, 8, NB, _cus(), 0x9 if KA // 32 == 20 else 0xF)
    return None if p is None else (p[0], p[1], B // p[0] // (32 * p[1]) * NB)


def bwd_plan(B, H):
    """launch_lstm_bwd_persistent (T >= 2): (nsub, units = NRT / 4, grid) or None."""
    if B % 64 or H not in (128, 256, 512) or B * 4 * H * 2 >= 2 ** 31 - 1:
        return None
    NB = H // 64
    p = persistent_split(B, 64, 4, NB, _cus(), 0xF)
    return None if p is None else (p[0], p[1], B // p[0] // (64 * p[1]) * NB)


def dw_uses_slab(G, KA, K, ksplit, slab_numel):
    """csrc/gemm.hip launch_gemm / launch_dw_288w: only the 256x288 tile (KA % 288 == 0) knows the
    slab; it clamps the split to one workgroup per CU, steps it down until 64 * nsplit divides K
    (equal_ksplit), and stores partials into the slab when more than one split remains and all of
    them fit (the engine's gW has ldo == KA). Otherwise fp32 atomics."""
    if KA % 288 or slab_numel is None:
        return False
    tiles = (G // 256) * (KA // 288)
    cus = _cus()
    ks = max(1, ksplit)
    if ks * tiles > cus and cus // tiles >= 1:
        ks = cus // tiles
    while ks > 1 and K % (64 * ks):
        ks -= 1
    return ks > 1 and ks * G * KA <= slab_numel and (G * KA) % 4 == 0


# ------------------------------------------------------------------ inputs of the accumulating calls
# The prior of the flat gradient bucket: sign x 2^e x (1 + k / 4096), k uniform in [0, 4096), one
# binade per segment of the bucket. Every element is nonzero (gW's padding columns included) and
# has 12 fraction bits, so its sum with an fp32 gradient of a nearby binade is far from exact: a
# kernel that adds must round, and one that stores drops a value 4x above the bound everywhere.
# The binades are chosen on the CPU from the emulation's float64 terms so that both teeth
# conditions of tests/test_lstm_steps_cpu.py::test_prior_has_teeth hold on its CASES (the figures
# are in that test's docstring).
PRIOR_EXP = {"gW": -15, "gw_out": -6, "gb_out": -4}
LOSS0 = 3.0  # the loss accumulator's preset


def lattice_prior(lay, seed=0, device="cpu"):
    """The flat bucket preset (float32 [lay.numel])."""
    g = torch.Generator().manual_seed(1000 + seed)
    k = torch.randint(0, 4096, (lay.numel,), generator=g).double()
    sign = torch.randint(0, 2, (lay.numel,), generator=g).double() * 2 - 1
    out = sign * (1 + k / 4096)
    W, w_out, b_out = lay.views(out)
    W *= 2.0 ** PRIOR_EXP["gW"]
    w_out *= 2.0 ** PRIOR_EXP["gw_out"]
    b_out *= 2.0 ** PRIOR_EXP["gb_out"]
    out[lay.w_size + lay.hidden + 1:] *= 2.0 ** PRIOR_EXP["gb_out"]  # the bucket's alignment tail
    f = out.float()
    assert torch.equal(f.double(), out) and bool((f != 0).all())
    return f.to(device)


def window_rows(B, T, F, seed=0, scale=1.0):
    """A row table of 3 B + T rows, 3 B overlapping windows over it (start = window id: neighbours
    share T - 1 rows), their targets, and three id vectors of B windows each: shuffled subsets with
    two ids repeated. -> (table [3B + T][F], starts [3B], yall [3B], [ids0, ids1, ids2])."""
    from wellflow.data.synth import synth_lstm_batch

    n = 3 * B + T
    x, _ = synth_lstm_batch(n // T + 1, T, F, seed=100 + seed)
    table = (x.float().reshape(-1, F)[:n] * scale).contiguous()
    g = torch.Generator().manual_seed(200 + seed)
    starts = torch.arange(3 * B, dtype=torch.int64)
    yall = torch.randn(3 * B, generator=g)
    ids = []
    for _ in range(3):
        v = torch.randperm(3 * B, generator=g)[:B].clone()
        v[B // 2], v[B - 1] = v[0], v[1]  # two windows twice in one batch
        ids.append(v)
    return table, starts, yall, ids


def gather_windows(table, starts, ids, T):
    """[B][T][F] = table[starts[ids] + t], on the host."""
    return table.cpu()[starts.cpu()[ids.cpu()][:, None] + torch.arange(T)[None, :]]
