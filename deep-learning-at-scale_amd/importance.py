"""Permutation feature importance: which of the submitted columns does a saved model use?

    python -m wellflow.importance <model> columnNames columnTypes targetColumn storagePath dataPath
                                  [--repeats R=5] [--columns a,b,..] [--out PATH] [--seed S] [--device D]
                                  [--precision P] [--seq-len T] [--group-col COL] [--batch-size B] [--header]

Shuffle ONE input column over the rows, score again, and report how much the error grows: the
model-agnostic answer to "could this column be dropped from the next submission". The data
should be HELD-OUT rows (rows the model was not fitted on): on training rows a column the model
merely memorised looks important. The raw column is what is permuted, so a categorical column's
whole one-hot block moves together: the importance is per submitted column.

A run is ``1 + columns x repeats`` scoring passes. On the native path (GPU, bf16) the raw columns
are uploaded once and every pass stays on the device: ``torch.randperm`` -> the assembly kernel
with one source column read through the permutation (csrc/features.hip) -> the engine's forward
into a device vector -> the fp64 error sums of that pass (csrc/score.hip) into its own slot. The
host reads the slots once, after the last pass. On the CPU / in fp32 the table column is permuted
on the host, ``FeaturePipeline.features`` builds the rows and the same error formula runs in numpy
float64: that path is the oracle of the native one.

Error of a pass, in raw target units, all in float64 (p: the network's output, y: the raw target):
``d = p * y_scale + y_shift - y``; ``mse = sum(d * d) / M``, ``mae = sum(|d|) / M``.
"""
from __future__ import annotations

import csv
import os
import sys

import numpy as np
import torch

from .models.gilbert import GilbertModel
from .predict import Predictor, _numeric_target, scoring_job
from .scoring import LstmPass, MlpPass, permuted

GILBERT_INPUTS = ("whp", "choke", "glr")
CSV_COLUMNS = ("column", "kind", "baseline_mse", "permuted_mse_mean", "permuted_mse_std", "importance", "ratio",
               "baseline_mae", "permuted_mae_mean")


class PermutationImportance:
    """``PermutationImportance(predictor, repeats, seed).run(table, columns=None, perms=None)``.

    ``perms`` injects the permutations, so two paths can be compared on identical shuffles: a
    tensor ``[len(columns)][repeats][N]`` or a callable ``(column name, repeat) -> perm [N]``. N
    is the table's row count; for the LSTM the permutation acts on the SERIES-SORTED row table
    (rows grouped into series as training grouped them, file order kept inside a series).
    Without ``perms`` they are drawn by ``torch.randperm`` from a ``torch.Generator`` seeded with
    ``seed`` on the device that scores, in (column, repeat) order.
    ``piece_rows``: rows of the assembled MLP table per piece on the native path (0 = what fits
    in 1/8 of HBM, as the prediction job; scoring.py); rounded down to whole engine batches."""

    def __init__(self, predictor: Predictor, repeats: int = 5, seed: int = 0, piece_rows: int = 0):
        if predictor.name == "cnn":
            raise ValueError("permutation importance does not apply to cnn: the CNN reads only the target's own "
                             "history, so there is no input column to permute")
        if int(repeats) < 1:
            raise ValueError(f"repeats must be >= 1, got {repeats}")
        self.pred, self.repeats, self.seed, self.piece_rows = predictor, int(repeats), int(seed), int(piece_rows)

    # ------------------------------------------------------------------ columns
    def input_columns(self) -> list:
        """[(name, kind)] of every column that can be permuted, in the assembly kernel's source
        order: the categorical columns (saved indexer order), then the continuous ones."""
        if self.pred.name == "gilbert":
            return [(c, "continuous") for c in GILBERT_INPUTS]
        pipe = self.pred.pipe
        return [(ix.column, "categorical") for ix in pipe.indexers] + [(c, "continuous") for c in pipe.continuous]

    def _select(self, columns):
        have = self.input_columns()
        if columns is None:
            return list(range(len(have)))
        names = [c for c, _ in have]
        picked = []
        for c in columns:
            if c not in names:
                what = ("gilbert reads only " + ", ".join(GILBERT_INPUTS)) if self.pred.name == "gilbert" else \
                    f"the model's input columns are {names}"
                raise ValueError(f"unknown column {c!r}: {what}")
            if names.index(c) in picked:
                raise ValueError(f"column {c!r} listed twice")
            picked.append(names.index(c))
        if not picked:
            raise ValueError("no column to permute")
        return picked

    def _target(self, table: dict) -> np.ndarray:
        tgt = self.pred.pipe.target if self.pred.pipe is not None else self.target
        if not tgt:
            raise ValueError("gilbert: name the target column (run(table, target=...))")
        if tgt not in table:
            raise ValueError(f"the data lacks the target column {tgt!r}: an importance is an error against it")
        y = _numeric_target(table, tgt)
        if y is None:
            raise ValueError(f"the target column {tgt!r} is not numeric")
        return y

    # ------------------------------------------------------------------ the run
    def run(self, table: dict, columns=None, perms=None, target: str | None = None) -> dict:
        """``target``: the target column's name (gilbert only; a learned model's saved pipeline
        knows its own)."""
        self.target = target
        pred = self.pred
        picked = self._select(columns)
        have = self.input_columns()
        n = len(next(iter(table.values()))) if table else 0
        if n < 1:
            raise ValueError("no rows to score")
        for c, _ in have:
            if c not in table:
                raise ValueError(f"the data lacks the input column {c!r}")
        y = self._target(table)
        R, K = self.repeats, len(picked)
        if isinstance(perms, torch.Tensor) or isinstance(perms, np.ndarray):
            perms = torch.as_tensor(perms)
            if tuple(perms.shape) != (K, R, n):
                raise ValueError(f"perms must be [{K}][{R}][{n}] (columns, repeats, rows), got {tuple(perms.shape)}")
        elif perms is not None and not callable(perms):
            raise TypeError("perms: a tensor [columns][repeats][rows] or a callable (column, repeat) -> perm")
        if pred.name == "gilbert":
            scorer = _GilbertScorer(pred, table, y)
        else:
            scorer = LearnedScorer(pred, table, y, self.piece_rows)
        if scorer.M < 1:
            raise ValueError(f"no row can be scored: every series is shorter than the window of {pred.seq_len} rows")
        gen = None
        if perms is None:
            gen = torch.Generator(device=scorer.perm_device)
            gen.manual_seed(self.seed)
        elif isinstance(perms, torch.Tensor):
            perms = scorer.own_perms(perms)  # one conversion / upload, in front of the pass loop
        scorer.begin(1 + K * R)
        with torch.no_grad():
            scorer.score(0, -1, None)
            for i, k in enumerate(picked):
                for r in range(R):
                    if gen is not None:
                        perm = torch.randperm(n, generator=gen, device=scorer.perm_device, dtype=scorer.perm_dtype)
                    elif callable(perms):
                        perm = scorer.own_perms(torch.as_tensor(perms(have[k][0], r)))
                        if perm.shape != (n,):
                            raise ValueError(f"perms({have[k][0]!r}, {r}) gave {tuple(perm.shape)}, not [{n}]")
                    else:
                        perm = perms[i, r]
                    scorer.score(1 + i * R + r, k, perm)
        sums = scorer.finish()  # float64 [1 + K * R][2]: the one read of the device
        M = scorer.M
        base_mse, base_mae = sums[0, 0] / M, sums[0, 1] / M
        rows = []
        for i, k in enumerate(picked):
            mse = sums[1 + i * R : 1 + (i + 1) * R, 0] / M
            mae = sums[1 + i * R : 1 + (i + 1) * R, 1] / M
            mean = float(mse.mean())
            # the mean of the differences, not the difference of the means: passes that equal the
            # baseline bit for bit (an unused column, the identity permutation) give exactly 0.0
            imp = float((mse - base_mse).mean())
            ratio = mean / base_mse if base_mse > 0 else (float("inf") if mean > 0 else float("nan"))
            rows.append({"column": have[k][0], "kind": have[k][1], "baseline_mse": float(base_mse),
                         "permuted_mse_mean": mean, "permuted_mse_std": float(mse.std()), "importance": imp,
                         "ratio": float(ratio), "baseline_mae": float(base_mae), "permuted_mae_mean": float(mae.mean()),
                         "permuted_mse": [float(v) for v in mse]})
        # descending; NaN (a NaN prediction: reported, not hidden) first; ties keep the column order
        rows.sort(key=lambda d: (0, 0.0) if np.isnan(d["importance"]) else (1, -d["importance"]))
        return {"model": pred.name, "native": bool(scorer.native), "rows": n, "scored": int(M), "repeats": R,
                "baseline_mse": float(base_mse), "baseline_mae": float(base_mae), "sums": sums, "importance": rows}


# ---------------------------------------------------------------------- scorers
def _err_sums_host(p, y64, y_scale: float, y_shift: float):
    """The error formula in numpy float64 (what csrc/score.hip computes on the device)."""
    d = np.asarray(p).astype(np.float64) * y_scale + y_shift - y64
    return float(np.sum(d * d)), float(np.sum(np.abs(d)))


class _Scorer:
    """One table, scored again and again with one column permuted. ``score(slot, k, perm)``
    leaves the pass's {sum d^2, sum |d|} in ``slot``; ``finish()`` returns them all."""

    native = False
    perm_device = torch.device("cpu")
    perm_dtype = torch.int64

    def own_perms(self, perms: torch.Tensor) -> torch.Tensor:
        return perms.to(self.perm_device, self.perm_dtype)

    def begin(self, passes: int) -> None:
        self.sums = np.zeros((passes, 2), np.float64)

    def finish(self) -> np.ndarray:
        return self.sums


class _GilbertScorer(_Scorer):
    def __init__(self, pred, table, y64):
        self.model = GilbertModel(correlation=pred.extra.get("correlation", "gilbert"))
        self.cols = {k: np.asarray(table[k], np.float64) for k in GILBERT_INPUTS}
        self.y, self.M = y64, len(y64)

    def score(self, slot, k, perm):
        cols = self.cols if k < 0 else permuted(self.cols, GILBERT_INPUTS[k], perm.numpy())
        self.sums[slot] = _err_sums_host(self.model.predict(cols), self.y, 1.0, 0.0)


class LearnedScorer(_Scorer):
    """The MLP and the LSTM: one pass of scoring.py per ``score``, then the error sums — on the
    device (csrc/score.hip) when the pass assembles there, else in numpy. LSTM: the column is
    permuted over the series-sorted row table; target: the raw target at each window's last row."""

    def __init__(self, pred, table, y64, piece_rows: int = 0):
        pipe = pred.pipe
        if pred.name == "lstm":
            ps = LstmPass(pred, table, "LSTM importance scoring")
        else:
            ps = MlpPass(pred, table, "MLP importance scoring", resident=True, piece_rows=piece_rows)
        self.pred, self.ps, self.M, self.native, self.on_device = pred, ps, ps.M, ps.native, ps.on_device
        self.y_scale, self.y_shift = (float(pipe.y_std), float(pipe.y_mean)) if pipe.standardize_target else (1.0, 0.0)
        self.y32 = y64.astype(np.float32)  # the kernel's target format; the oracle scores against the same values
        if ps.rows is not None:
            self.y32 = self.y32[ps.rows]
        self.y64 = self.y32.astype(np.float64)
        if self.on_device:
            from .ops.native import err_sums_scratch

            self.perm_device, self.perm_dtype = pred.device, torch.int32
            self.scratch = err_sums_scratch(pred.device)
            self.y_dev = torch.from_numpy(self.y32).to(pred.device)

    def begin(self, passes):
        if self.on_device:
            self.out = torch.zeros((passes, 2), dtype=torch.float64, device=self.pred.device)
        else:
            super().begin(passes)

    def finish(self):
        self.pred.eng.check_device_errors()
        return self.out.cpu().numpy() if self.on_device else self.sums

    def reduce(self, slot):
        from .ops.native import err_sums

        err_sums(self.ps.p, self.y_dev, self.y_scale, self.y_shift, self.out, slot, self.scratch)

    def score(self, slot, k, perm):
        p = self.ps.score(k, perm)
        if self.on_device:
            self.reduce(slot)
        else:
            self.sums[slot] = _err_sums_host(torch.as_tensor(p).cpu().numpy(), self.y64, self.y_scale, self.y_shift)


# ---------------------------------------------------------------------- the job
def _write_csv(path: str, rows: list) -> None:
    """One row per column, most important first; always with a header. Atomic (tmp + rename)."""
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    tmp = path + ".tmp"
    with open(tmp, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(CSV_COLUMNS)
        for d in rows:
            w.writerow([d[c] if isinstance(d[c], str) else repr(float(d[c])) for c in CSV_COLUMNS])
    os.replace(tmp, path)


def run_importance(model: str, argv, log=print) -> dict:
    def add_arguments(ap):
        ap.add_argument("--repeats", type=int, default=5, help="shuffles per column (default 5)")
        ap.add_argument("--columns", default=None, help="comma-separated input columns (default: all)")

    ns, cfg, schema, out_path, load_predictor, load_data = scoring_job(
        "importance", "importance", "importance", "dataPath (the data: held-out rows)", model, argv, add_arguments)
    if int(os.environ.get("RANK", "0")) != 0:  # one process on one device: rank 0 alone works and writes
        return {"model": model, "out": out_path, "skipped": True}
    job = PermutationImportance(load_predictor(), repeats=ns.repeats, seed=cfg.seed)
    table = load_data()
    columns = [c.strip() for c in ns.columns.split(",") if c.strip()] if ns.columns is not None else None
    result = job.run(table, columns=columns, target=cfg.target)
    result["out"] = out_path
    _write_csv(out_path, result["importance"])
    log("Rows scored: %d" % result["scored"])
    log("Baseline MSE: %f" % result["baseline_mse"])
    for d in result["importance"]:
        log("%s (%s): importance %f, ratio %f" % (d["column"], d["kind"], d["importance"], d["ratio"]))
    return result


def main(argv=None) -> int:
    argv = list(sys.argv[1:] if argv is None else argv)
    if not argv or argv[0] in ("-h", "--help"):
        print(__doc__)
        return 0
    run_importance(argv[0], argv[1:])
    return 0


if __name__ == "__main__":
    sys.exit(main())
