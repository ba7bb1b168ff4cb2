"""Training loop (replaces Keras ``model.fit`` + callbacks, cnn.py:121-134).

Semantics kept from the reference (Keras 0.x):
* per-epoch shuffle, ``verbose=2`` one line per epoch;
* ``EarlyStopping(monitor='val_loss', patience=10)`` with Keras-0.1's exact rule (the
  wait counter is checked BEFORE it is incremented, so training stops after
  patience + 1 non-improving epochs);
* ``ModelCheckpoint(..., save_best_only=True)`` -> ``<storagePath>models/<name>.mdl``
  written when val_loss < best;
* wall time around fit, one evaluation pass on the test split, and the two final stdout
  lines ``Time elapsed: %f s`` / ``Testing set loss: %f`` (fixed for Python 3).

Added for the MI355X engine: one process per GPU (DistContext), per-epoch seeded shuffle
identical on every rank then a disjoint rank shard (DistributedSampler semantics), the
whole dataset RESIDENT in HBM (indexed on device, no per-step host copies), one flat
gradient all-reduce per step (C2), all-reduced val metrics so every rank takes the same
early-stop decision (C3), rank-0 checkpoint writes fenced by barriers (C4), a resumable
``.ckpt`` each epoch, and env/flag fault injection (``WELLFLOW_FAIL_AT_STEP``) to test it.
"""
from __future__ import annotations

import dataclasses
import json
import math
import os
import time

import numpy as np
import torch

from ..models.base import CLIP_STEPS_REASON, note_slow_path, per_element_loss
from ..utils import checkpoint as ckpt
from ..utils.profiling import trace_range


class InjectedFault(RuntimeError):
    pass


@dataclasses.dataclass
class EarlyStopping:
    patience: int = 10
    best: float = math.inf
    wait: int = 0
    stopped: bool = False

    def update(self, current: float) -> bool:
        """Keras-0.1 rule; returns True when training must stop."""
        if current < self.best:
            self.best = current
            self.wait = 0
        else:
            if self.wait >= self.patience:
                self.stopped = True
            self.wait += 1
        return self.stopped


@dataclasses.dataclass
class History:
    loss: list = dataclasses.field(default_factory=list)
    val_loss: list = dataclasses.field(default_factory=list)
    val_mse: list = dataclasses.field(default_factory=list)
    epoch_time: list = dataclasses.field(default_factory=list)
    # wall (host) clock around an epoch's / chunk's training steps: from before the first
    # launch to after the final synchronize, so host issue gaps count (round-4 VERDICT item 8:
    # the primary figure)
    rows_per_s: list = dataclasses.field(default_factory=list)
    # the device's busy span for the same steps (CUDA events on the compute stream), beside it
    rows_per_s_device: list = dataclasses.field(default_factory=list)


class StepClock:
    """Times a run of training steps: CUDA events on the compute stream around the launches
    (the first event right before the first step is issued, the last after the last one), so
    the figure is the device's busy span for those steps, independent of host hiccups at the
    boundaries (an 8-step stream chunk is ~2 ms: one 0.4 ms host stall at its start read as
    a 20 % slower chunk); the host clock is kept beside it."""

    def __init__(self, device):
        self.cuda = torch.device(device).type == "cuda"
        self.device = device
        self.t0 = time.perf_counter()
        self.ev0 = self.ev1 = None

    def first(self) -> None:
        if self.cuda and self.ev0 is None:
            self.ev0 = torch.cuda.Event(enable_timing=True)
            self.ev0.record(torch.cuda.current_stream(self.device))

    def stop(self):
        """-> (device seconds or host seconds off-GPU, host seconds); synchronizes."""
        if self.cuda:
            if self.ev0 is not None:
                self.ev1 = torch.cuda.Event(enable_timing=True)
                self.ev1.record(torch.cuda.current_stream(self.device))
            torch.cuda.synchronize(self.device)
        host = time.perf_counter() - self.t0
        if self.ev0 is None:
            return host, host
        return self.ev0.elapsed_time(self.ev1) / 1e3, host


def _graph_steps() -> int:
    """Training steps per graph replay in the resident-data loop (WELLFLOW_GRAPH_STEPS, default 8)."""
    try:
        return max(1, int(os.environ.get("WELLFLOW_GRAPH_STEPS", "8")))
    except ValueError:
        return 8


# The pre-permuted (sliced) epoch path keys its captured graphs by step offset: one graph per
# aligned n-step group plus the singles, all kept for the job. Above this many steps per epoch
# (the job default batch 256 on a multi-million-row table: thousands) the epoch takes the
# row-indexed path instead, whose graphs are keyed by n only (round-5 ADVICE).
MAX_SLICED_STEPS = 128
# steps per persistent small-batch launch (NativeMLP.fused_steps): one ~5-us launch per this many
# steps; the Trainer's per-step bookkeeping runs on the host after each launch
SMALL_STEPS_PER_LAUNCH = 256


def _resident_windows(X, device) -> bool:
    rows = getattr(X, "rows", None)
    if not (torch.is_tensor(rows) and torch.is_tensor(getattr(X, "starts", None))):
        return False
    same = rows.device.type == device.type and (device.index is None or rows.device.index in (None, device.index))
    return same and rows.is_cuda and rows.dtype == torch.float32 and rows.is_contiguous() and rows.dim() == 2


def small_steps_path(eng, opt, ctx, cfg, b: int, X):
    """Whether batches of ``b`` rows of ``X`` may train K steps per persistent launch
    (Engine.fused_steps) -> (eligible, the engine's reason; None when it was not asked): one
    process (the update inside the launch has no all-reduce), no per-step fault injection, and
    nothing against it from the engine. Clipping alone in the way (engines check it last) is said once."""
    if ctx.world_size != 1 or cfg.fail_at_step >= 0:
        return False, None
    why = eng.small_steps_reason(b, opt, X)
    if why == CLIP_STEPS_REASON:
        note_slow_path(type(eng).__name__, "training runs one update per step, not K steps per launch",
                       why, f"B={b}")
    return why is None, why


def _to_dev(a, device):
    if hasattr(a, "to") and hasattr(a, "starts"):  # data.features.SeriesWindows: rows + starts
        return a.to(device)
    t = torch.as_tensor(a)
    if t.dtype == torch.float64:
        t = t.float()
    return t.to(device)


class Trainer:
    def __init__(self, cfg, engine, optimizer, ctx, name: str, on_best=None, n_outputs: int = 1,
                 log=print):
        self.cfg, self.eng, self.opt, self.ctx = cfg, engine, optimizer, ctx
        self.name, self.on_best, self.n_out = name, on_best, n_outputs
        self.log = log if ctx.is_main else (lambda *a, **k: None)
        self.history = History()
        self.stopper = EarlyStopping(cfg.patience)
        self.epoch = 0
        self.global_step = 0
        self.extra_state = {}
        self._runners = {}
        self._idx = {}

    # ------------------------------------------------------------------ helpers
    def _local_batch(self, n_train: int) -> int:
        per_rank = n_train // max(self.ctx.world_size, 1)
        return max(1, min(self.cfg.batch_size, per_rank))

    def resident(self, X, Y):
        """(X, Y) of an evaluation split as device tensors in the engine's input format, cached
        per split, for native GPU engines on plain arrays (the small well-log sets fit HBM whole);
        anything else comes back unchanged. Evaluating from host arrays cost ~220 ms per MLP
        epoch of 7 ms of training (a numpy gather + copy + two syncs per chunk)."""
        eng = self.eng
        if not (eng.native and eng.device.type == "cuda"):
            return X, Y
        key = ("resident", id(X), id(Y))
        hit = self._idx.get(key)
        if hit is not None and hit[0] is X and hit[1] is Y:
            return hit[2], hit[3]
        rows = getattr(X, "rows", X)  # windows: their row table is what moves
        nbytes = getattr(rows, "nbytes", 0) or (rows.numel() * rows.element_size() if torch.is_tensor(rows) else 0)
        if nbytes > torch.cuda.get_device_properties(eng.device).total_memory // 8:
            return X, Y  # a split this large stays on the host (chunked path)
        Xd, Yd = _to_dev(X, eng.device), _to_dev(Y, eng.device)  # windows: rows + starts on the device
        Xd = eng.to_input_format(Xd) if torch.is_tensor(Xd) else Xd  # (window sets stay as they are)
        self._idx[key] = (X, Y, Xd, Yd)
        return Xd, Yd

    def evaluate(self, X, Y, chunk: int | None = None):
        """-> (mean training-loss, mean MSE) over the split, all-reduced across ranks."""
        n = len(X)
        if n == 0:
            return float("nan"), float("nan")
        X, Y = self.resident(X, Y)
        w, r = self.ctx.world_size, self.ctx.rank
        dev = self.eng.device
        if torch.is_tensor(Y) and Y.device == dev and getattr(X, "device", None) == dev:
            return self._eval_device(X, Y, w, r, chunk)
        idx = np.arange(r, n, w)
        chunk = chunk or self.eng.B or 4096
        Xd = X if (torch.is_tensor(X) or hasattr(X, "starts")) and getattr(X, "device", None) == self.eng.device \
            else None
        pf = self._eval_prefetcher(X, chunk) if Xd is None and len(idx) > chunk else None
        try:
            s_loss, s_mse, cnt = self._eval_chunks(X, Y, Xd, idx, chunk, pf)
        finally:  # the gather threads and slot buffers go away on the error path too
            if pf is not None:
                pf.close()
        s_loss, s_mse, cnt = self.ctx.sum_scalars(s_loss, s_mse, cnt)
        return s_loss / max(cnt, 1), s_mse / max(cnt, 1)

    def _eval_device(self, X, Y, w: int, r: int, chunk: int | None):
        """Device-resident split: rank r's rows r, r + w, ... as strided slices (no gather; a
        window set gathers each chunk's windows on the GPU), the sums accumulated on the device
        and read back once."""
        chunk = chunk or self.eng.B or 4096
        windows = hasattr(X, "starts")  # device windows: each chunk gathered on the GPU
        ridx = torch.arange(r, len(X), w, device=Y.device) if windows else None
        Xr, Yr = (X, Y[r::w]) if windows else (X[r::w], Y[r::w])
        acc = torch.zeros(2, dtype=torch.float64, device=Y.device)
        for i in range(0, len(Yr), chunk):
            xb = X[ridx[i : i + chunk]] if windows else Xr[i : i + chunk]
            yb = Yr[i : i + chunk]
            if not xb.is_contiguous():
                xb = xb.contiguous()
            yb = yb.float()
            pred = self.eng.forward(xb).float().reshape(yb.shape)
            acc[0] += per_element_loss(self.cfg.loss, pred, yb, self.cfg.clip).sum()
            acc[1] += ((pred - yb) ** 2).sum()
        s_loss, s_mse = acc.tolist()
        s_loss, s_mse, cnt = self.ctx.sum_scalars(s_loss, s_mse, float(Yr.numel()))
        return s_loss / max(cnt, 1), s_mse / max(cnt, 1)

    def _eval_chunks(self, X, Y, Xd, idx, chunk, pf):
        s_loss, s_mse, cnt = 0.0, 0.0, 0
        if pf is not None:
            pf.submit(0, idx[:chunk])
        for k, i in enumerate(range(0, len(idx), chunk)):
            sel = idx[i : i + chunk]
            if pf is not None:
                # native background gather (csrc/runtime: wf_prefetch_*) of the next chunk's
                # windows into the other slot while this chunk is copied and evaluated
                if i + chunk < len(idx):
                    pf.submit((k + 1) % 2, idx[i + chunk : i + 2 * chunk])
                xh, _ = pf.wait(k % 2)
                xb = xh.to(self.eng.device)  # synchronous: the slot is free again afterwards
            else:
                xb = (Xd[torch.as_tensor(sel, device=Xd.device)] if Xd is not None
                      else _to_dev(X[sel], self.eng.device))
            yb = _to_dev(Y[sel] if not torch.is_tensor(Y) else Y[torch.as_tensor(sel, device=Y.device)],
                         self.eng.device)
            pred = self.eng.forward(xb).float().reshape(yb.shape)
            s_loss += per_element_loss(self.cfg.loss, pred, yb, self.cfg.clip).sum().item()
            s_mse += ((pred - yb) ** 2).sum().item()
            cnt += yb.numel()
        return s_loss, s_mse, cnt

    def _eval_prefetcher(self, X, chunk: int):
        """Two-slot native window prefetcher for a host-resident window set (float32
        SeriesWindows rows), or None (tensor / other storage, native runtime not built)."""
        from ..data import native

        rows = getattr(X, "rows", None)
        if not (hasattr(X, "starts") and isinstance(rows, np.ndarray) and rows.dtype == np.float32
                and native.wanted()):
            return None
        # targets come from Y per window; the prefetcher's per-row target buffer is unused.
        # Pageable slots by default (WELLFLOW_EVAL_PIN=1: pinned). Round 2 saw pinned slots
        # break graph-replayed persistent launches; the cause was the per-launch memset of the
        # sync words (profiles/r3_early_exit.md), fixed, and tests/test_job_gpu.py runs both.
        # Pinned measured no faster for evaluation (1.69 vs 1.70 M rows/s job).
        return native.Prefetcher(rows, np.asarray(X.starts), np.zeros(len(rows), np.float32), X.T, chunk,
                                 nslots=2, threads=2, pin=os.environ.get("WELLFLOW_EVAL_PIN", "0") == "1")

    # ------------------------------------------------------------------ state
    def state_dict(self) -> dict:
        return {
            "name": self.name,
            "epoch": self.epoch,
            "global_step": self.global_step,
            "params": self.eng.params.detach().cpu().clone(),
            # (optimizer.state_dict reads the device step counter: graph replays advance it)
            "optimizer": self.opt.state_dict(),
            "early_stopping": dataclasses.asdict(self.stopper),
            "history": dataclasses.asdict(self.history),
            "extra": self.extra_state,
            "numpy_seed": int(self.cfg.seed),
            "layout": self._layout_tag(),
        }

    def _layout_tag(self) -> dict:
        """What the flat parameter vector means: its length and the engine's layout (e.g. the
        CNN's padded filter count), checked on resume (round-4 ADVICE: a layout change used to
        surface as a bare size mismatch inside params.copy_)."""
        return {"engine": type(self.eng).__name__, "numel": int(self.eng.params.numel()),
                "layout": repr(self.eng.lay) if self.eng.lay is not None else None}

    def load_state_dict(self, sd: dict) -> None:
        mine, theirs = self._layout_tag(), sd.get("layout")
        if sd["params"].numel() != mine["numel"] or (theirs and theirs.get("layout") and mine["layout"]
                                                     and theirs["layout"] != mine["layout"]):
            raise ValueError(
                f"checkpoint parameter layout does not match this engine: checkpoint {theirs or 'untagged'} "
                f"with {sd['params'].numel()} values, engine {mine}. It was written by a different model "
                "configuration or an older flat layout; start without --resume (or remap the weights).")
        self.eng.params.copy_(sd["params"].to(self.eng.params.device))
        self.eng.sync_weights()
        if self.eng.rng is not None:  # dropout stream continues where it stopped
            self.eng.rng.fill_(int(sd["global_step"]))
        self.opt.load_state_dict(sd["optimizer"])
        self.epoch = int(sd["epoch"])
        self.global_step = int(sd["global_step"])
        es = sd["early_stopping"]
        self.stopper = EarlyStopping(int(es["patience"]), float(es["best"]), int(es["wait"]),
                                     bool(es["stopped"]))
        known = {f.name for f in dataclasses.fields(History)}  # (rows_per_s_host: pre-round-5 name)
        self.history = History(**{k: list(v) for k, v in sd["history"].items() if k in known})
        self.extra_state = dict(sd.get("extra", {}))

    def try_resume(self) -> bool:
        path = self.cfg.ckpt_path(self.name)
        if not (self.cfg.resume and os.path.exists(path)):
            return False
        self.load_state_dict(ckpt.load_state(path))
        self.log(f"Resumed from {path} at epoch {self.epoch} (step {self.global_step})")
        return True

    def save_state(self) -> None:
        self.ctx.barrier()
        if self.ctx.is_main:
            ckpt.save_state(self.cfg.ckpt_path(self.name), self.state_dict())
        self.ctx.barrier()

    # ------------------------------------------------------------------ faults / metrics
    def _inject_fault(self) -> None:
        """Fail ONCE per (storage path, model, rank): a marker file makes the restarted
        process (torchrun --max-restarts, or a manual --resume) run through."""
        d = self.cfg.model_dir
        os.makedirs(d, exist_ok=True)
        marker = os.path.join(d, f".fault_injected_{self.name}_r{self.ctx.rank}")
        if os.path.exists(marker):
            return
        with open(marker, "w") as f:
            f.write(str(self.global_step))
        raise InjectedFault(f"injected fault at step {self.global_step}")

    def _log_metrics(self) -> None:
        path = getattr(self.cfg, "metrics_path", "")
        if not path or not self.ctx.is_main:
            return
        h = self.history
        rec = {"epoch": self.epoch, "global_step": self.global_step, "loss": h.loss[-1],
               "val_loss": h.val_loss[-1], "val_mse": h.val_mse[-1], "rows_per_s": h.rows_per_s[-1],
               "epoch_time_s": h.epoch_time[-1], "world_size": self.ctx.world_size,
               "time": time.time()}
        if getattr(self.opt, "clips", False):  # gradient norms of this epoch's steps (optim/flat.py clip_stats)
            rec.update(self.opt.clip_stats(reset=True))
        with open(path, "a") as f:
            f.write(json.dumps(rec) + "\n")

    # ------------------------------------------------------------------ fit
    def _runner(self, key, make_inputs, b: int):
        """The StepRunner (train/step.py, the same step bench.py times) for batches of ``b``
        rows, cached per data source: after two eager steps it replays as one hipGraph."""
        from .step import StepRunner

        rk = (key, b)
        if self._runners.get("key") != rk:
            gscale = 1.0 / (b * self.ctx.world_size * self.n_out)
            self._runners = {"key": rk, "run": StepRunner(self.eng, self.opt, self.ctx, gscale, make_inputs,
                                                          graph=None if self.eng.native else False)}
        return self._runners["run"]

    def _after_step(self) -> bool:
        """Step bookkeeping; True = stop (max_steps)."""
        self.global_step += 1
        cfg = self.cfg
        if cfg.fail_at_step >= 0 and self.global_step == cfg.fail_at_step:
            self._inject_fault()
        return bool(cfg.max_steps and self.global_step >= cfg.max_steps)

    def _epoch_order(self, n: int, per_rank: int, dev):
        """This rank's rows of the epoch's shuffle (seed + 7919 * epoch, the same on every rank).
        On a GPU the permutation is drawn on the device (torch.randperm with a seeded device
        generator): the host numpy permutation + 78-MB index copy took ~200 ms per epoch of a
        15 M-row table (the MLP job's epochs train for 7 ms)."""
        cfg, ctx = self.cfg, self.ctx
        seed = cfg.seed + 7919 * self.epoch
        if torch.device(dev).type == "cuda":
            g = torch.Generator(device=dev)
            g.manual_seed(seed)
            perm = torch.randperm(n, generator=g, device=dev)
            return perm[ctx.rank * per_rank : (ctx.rank + 1) * per_rank]
        perm = np.random.default_rng(seed).permutation(n)
        return torch.as_tensor(perm[ctx.rank * per_rank : (ctx.rank + 1) * per_rank], device=dev)

    def _permuted(self, Xd, Yd, order):
        """The epoch's shuffle materialised: this rank's rows gathered once, in ``order``, into
        persistent device buffers (two row-gather launches per epoch), so each step reads its
        batch as a contiguous slice instead of one 32-B row at a random address per batch row
        (the MLP job ran at 0.75 of the resident-batch bench that way). Only for row-indexed
        engines on a GPU and while the copy takes under a quarter of the device's memory; None =
        keep gathering from the dataset in place."""
        eng = self.eng
        if not (eng.row_indexed and torch.is_tensor(Xd) and torch.is_tensor(Yd) and Xd.device.type == "cuda"):
            return None
        m = len(order)
        need = m * (Xd[0].numel() * Xd.element_size() + Yd[0].numel() * Yd.element_size())
        if need > torch.cuda.get_device_properties(Xd.device).total_memory // 4:
            return None
        key = ("perm", Xd.dtype, Yd.dtype, tuple(Xd.shape[1:]), tuple(Yd.shape[1:]), m)
        bufs = self._idx.get(key)
        if bufs is None:
            bufs = self._idx[key] = (torch.empty((m,) + tuple(Xd.shape[1:]), dtype=Xd.dtype, device=Xd.device),
                                     torch.empty((m,) + tuple(Yd.shape[1:]), dtype=Yd.dtype, device=Yd.device))
        eng.gather_rows(Xd, order, bufs[0])
        eng.gather_rows(Yd, order, bufs[1])
        return bufs

    def train_steps(self, Xd, Yd, order: torch.Tensor, b: int, sliced: bool = False):
        """One pass over ``order`` (device index tensor of this rank) in batches of ``b``.

        Each step gathers its batch from the resident dataset through a STATIC index buffer
        inside the captured step, so the whole step (gather, fwd, bwd, all-reduce, update)
        is one graph replay; the remainder that does not fill a batch is dropped (the native
        engines run fixed-shape batches). ``sliced``: Xd / Yd already hold the pass's rows in
        order (Trainer._permuted): step j reads rows j*b .. (j+1)*b - 1 as a contiguous slice,
        a fixed address per step, so every step's graph is captured once and no index is read."""
        eng, ctx = self.eng, self.ctx
        steps = len(order) // b
        if steps == 0 and len(order) > 0 and not eng.native:
            steps, b = 1, len(order)
        idx = self._idx.get(b)
        if idx is None:
            idx = self._idx[b] = torch.zeros(b, dtype=torch.long, device=eng.device)

        row_indexed = eng.row_indexed and torch.is_tensor(Xd)
        # resident windows (SeriesWindows on the device) that the engine reads in place through
        # the step's window ids (NativeLSTM: the x-pack kernel gathers them)
        row_indexed = row_indexed or (eng.window_indexed and _resident_windows(Xd, eng.device))
        # groups of n steps as ONE graph replay (StepRunner.run_many): step i of a group reads its
        # rows from slice i of a static order buffer filled by one copy per group; the per-step
        # index copy + replay gap (~8 us of a 165-us MLP step) goes away. Row-indexed engines,
        # no per-step fault injection.
        n_many = (_graph_steps() if ((row_indexed or sliced) and eng.device.type == "cuda" and self.cfg.fail_at_step < 0)
                  else 1)
        if n_many > 1 and steps > 1:  # balanced groups: 9 steps run as one 9-step replay, not 8 + 1
            groups = max(1, round(steps / n_many))
            n_many = -(-steps // groups)
        ordbuf = None
        if n_many > 1 and steps >= n_many and not sliced:
            ordbuf = self._idx.get(("many", b, n_many))
            if ordbuf is None:
                ordbuf = self._idx[("many", b, n_many)] = torch.zeros(n_many * b, dtype=torch.long, device=eng.device)

        def inputs(k):
            if sliced:  # step j = k (single) or k[0] + k[1] (step k[1] of the group starting at k[0])
                j = k[0] + k[1] if isinstance(k, tuple) else k
                return Xd[j * b : (j + 1) * b], Yd[j * b : (j + 1) * b]
            if row_indexed:  # the engine's kernels read the rows through the index
                if isinstance(k, tuple):  # step k[1] of a run_many group
                    return Xd, Yd, ordbuf[k[1] * b : (k[1] + 1) * b]
                return Xd, Yd, idx
            if torch.is_tensor(Xd):  # row gather (index_select: one coalesced kernel per tensor)
                return Xd.index_select(0, idx), Yd.index_select(0, idx)
            return Xd[idx], Yd.index_select(0, idx)

        run = self._runner(("resident", id(Xd), id(Yd)), inputs, b)
        if run.loss_acc is not None:
            run.loss_acc.zero_()  # no take_loss() here: its sync left the GPU idle through the first launch
        clock = StepClock(eng.device)
        done = 0
        cfg = self.cfg
        s = 0
        prepared = False
        # small batches (the job defaults: MLP 256 rows, CNN 20 windows): up to
        # SMALL_STEPS_PER_LAUNCH complete steps — forward, backward AND the optimizer update — per
        # persistent launch (NativeMLP / NativeCNN.fused_steps, csrc/mlp_small.hip, cnn_small.hip)
        small, _ = small_steps_path(eng, self.opt, ctx, cfg, b, Xd)
        while small and s < steps:
            clock.first()
            n = min(steps - s, SMALL_STEPS_PER_LAUNCH)
            if cfg.max_steps:
                n = max(0, min(n, cfg.max_steps - self.global_step))
            if n == 0:
                break
            gscale = 1.0 / (b * ctx.world_size * self.n_out)
            if sliced:
                eng.fused_steps(Xd[s * b : (s + n) * b], Yd[s * b : (s + n) * b], b, n, self.opt, gscale,
                                loss_into=run.loss_acc)
            else:
                eng.fused_steps(Xd, Yd, b, n, self.opt, gscale, rows=order[s * b : (s + n) * b],
                                loss_into=run.loss_acc)
            stop = False
            for _ in range(n):
                stop = self._after_step() or stop
            done += n
            s += n
            if stop:
                break
        while not small and s < steps:
            clock.first()
            n = n_many
            if sliced and n > 1 and not prepared and run.calls > run.eager_steps + 1:
                # every aligned group's graph (starts 0, n, 2n, ...) captured up front, in the first
                # epoch: later epochs replay only, none of them pays a capture
                prepared = all(run.prepare_many(n, g0) for g0 in range(0, steps - n + 1, n))
            if ((ordbuf is None and not sliced) or n <= 1 or s + n > steps or run.calls <= run.eager_steps + 1
                    or (sliced and s % n != 0)
                    or (cfg.max_steps and self.global_step + n > cfg.max_steps)):
                if sliced:
                    run.run(s)
                else:
                    idx.copy_(order[s * b : (s + 1) * b])
                    run.run()
                n = 1
            elif sliced:
                run.run_many(n, s)
            else:
                ordbuf.copy_(order[s * b : (s + n) * b])
                run.run_many(n)
            stop = False
            for _ in range(n):
                stop = self._after_step() or stop
            done += n
            s += n
            if stop:
                break
        dt, self.last_host_dt = clock.stop()
        (tot,) = ctx.sum_scalars(run.take_loss())
        rows = done * b * ctx.world_size
        return tot / max(rows * self.n_out, 1), rows, dt

    def fit(self, train, val):
        cfg, ctx = self.cfg, self.ctx
        Xtr, Ytr = train
        dev = self.eng.device
        # resident dataset in device memory (288 GB HBM: the small well-log sets fit whole)
        Xd, Yd = _to_dev(Xtr, dev), _to_dev(Ytr, dev)
        Xd = self.eng.to_input_format(Xd) if torch.is_tensor(Xd) else Xd  # (NativeMLP: bf16 [N][Fp], read in place)
        n = len(Xd)
        b = self._local_batch(n)
        per_rank = n // max(ctx.world_size, 1)
        while self.epoch < cfg.epochs and not self.stopper.stopped:
            t_ep = time.perf_counter()
            order = self._epoch_order(n, per_rank, dev)
            src = self._permuted(Xd, Yd, order) if per_rank // max(b, 1) <= MAX_SLICED_STEPS else None
            if src is not None:  # this epoch's rows in shuffled order, read as contiguous slices
                Xs, Ys = src
            else:
                Xs, Ys = Xd, Yd
            with trace_range("train_epoch", dev):
                tr_loss, rows, dt = self.train_steps(Xs, Ys, order, b, sliced=src is not None)
            self.eng.check_device_errors()  # once per epoch: a hand-off timed out in some step
            with trace_range("evaluate", dev):
                v_loss, v_mse = self.evaluate(*val)
            self.epoch += 1
            h = self.history
            h.loss.append(tr_loss)
            h.val_loss.append(v_loss)
            h.val_mse.append(v_mse)
            h.epoch_time.append(time.perf_counter() - t_ep)
            hd = getattr(self, "last_host_dt", dt)
            h.rows_per_s.append(rows / hd if hd > 0 else 0.0)
            h.rows_per_s_device.append(rows / dt if dt > 0 else 0.0)
            if cfg.verbose >= 2:
                self.log(f"Epoch {self.epoch}/{cfg.epochs} - {h.epoch_time[-1]:.2f}s - loss: {tr_loss:.6f}"
                         f" - val_loss: {v_loss:.6f} - val_mse: {v_mse:.6f} - rows/s: {h.rows_per_s[-1]:.0f}",
                         flush=True)
            self._log_metrics()
            improved = v_loss < self.stopper.best
            self.stopper.update(v_loss)
            with trace_range("checkpoint", dev):
                if improved and self.on_best is not None:
                    ctx.barrier()
                    if ctx.is_main:
                        self.on_best(self)
                    ctx.barrier()
                self.save_state()
            if cfg.max_steps and self.global_step >= cfg.max_steps:
                break
        return self.history
