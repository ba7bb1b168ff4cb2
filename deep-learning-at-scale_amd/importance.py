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

import sys

import numpy as np
import torch

from .predict import Predictor, _numeric_target, scoring_job
from .scoring import PermutedColumn
from .whatif import Permutations, comma_list, input_columns, other_rank, scorer_for, select_columns, table_rows, write_csv

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

    def input_columns(self) -> list:
        """[(name, kind)] of every column that can be permuted, in the assembly kernel's source
        order: the categorical columns (saved indexer order), then the continuous ones."""
        return input_columns(self.pred)

    def _target(self, table: dict, target) -> np.ndarray:
        tgt = self.pred.pipe.target if self.pred.pipe is not None else target
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
        pred = self.pred
        picked = select_columns(pred, columns, "no column to permute")
        have = self.input_columns()
        n = table_rows(pred, table)
        y = self._target(table, target)
        R, K = self.repeats, len(picked)
        perms = Permutations(perms, (K, R, n), "columns, repeats, rows", "(column, repeat)")
        scorer = scorer_for(pred, table, "importance", self.piece_rows)
        perms.bind(scorer, self.seed)
        err = ErrorSums(scorer, y)
        err.begin(1 + K * R)
        with torch.no_grad():
            err.score(0)
            for i, k in enumerate(picked):
                for r in range(R):
                    err.score(1 + i * R + r, PermutedColumn(k, perms.draw((i, r), (have[k][0], r))))
        sums = err.finish()  # float64 [1 + K * R][2]: the one read of the device
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


# ---------------------------------------------------------------------- the reduction
def _err_sums_host(p, y64, y_scale: float, y_shift: float):
    """The error formula in numpy float64 (what csrc/score.hip computes on the device)."""
    d = np.asarray(p).astype(np.float64) * y_scale + y_shift - y64
    return float(np.sum(d * d)), float(np.sum(np.abs(d)))


class ErrorSums:
    """``score(slot, edit)`` scores the edited table (whatif.py) and leaves the pass's
    {sum d^2, sum |d|} in ``slot``; ``finish()`` returns them all. The sums are formed on the device
    (csrc/score.hip) when the pass ASSEMBLES there (the target is uploaded next to the raw
    columns), else in numpy. A learned model is scored against the target in the kernel's format,
    fp32, on both paths, at each prediction's row (LSTM: its window's last row)."""

    def __init__(self, scorer, y64: np.ndarray):
        self.scorer, self.device = scorer, scorer.on_device
        if scorer.learned:
            y32 = y64.astype(np.float32)
            y32 = y32 if scorer.rows is None else y32[scorer.rows]
            y64 = y32.astype(np.float64)
        self.y64 = y64
        if self.device:
            from .ops.native import err_sums_scratch

            self.scratch = err_sums_scratch(scorer.pred.device)
            self.y_dev = torch.from_numpy(y32).to(scorer.pred.device)

    def begin(self, passes: int) -> None:
        if self.device:
            self.out = torch.zeros((passes, 2), dtype=torch.float64, device=self.scorer.pred.device)
        else:
            self.sums = np.zeros((passes, 2), np.float64)

    def reduce(self, slot: int) -> None:
        from .ops.native import err_sums

        s = self.scorer
        err_sums(s.ps.p, self.y_dev, s.y_scale, s.y_shift, self.out, slot, self.scratch)

    def score(self, slot: int, edit=None) -> None:
        s = self.scorer
        p = s.predict(edit)
        if self.device:
            self.reduce(slot)
        else:
            self.sums[slot] = _err_sums_host(torch.as_tensor(p).cpu().numpy(), self.y64, s.y_scale, s.y_shift)

    def finish(self) -> np.ndarray:
        self.scorer.check_device_errors()
        return self.out.cpu().numpy() if self.device else self.sums


# ---------------------------------------------------------------------- the job
def _write_csv(path: str, rows: list) -> None:
    """One row per column, most important first; always with a header."""
    write_csv(path, CSV_COLUMNS, ([d[c] if isinstance(d[c], str) else repr(float(d[c])) for c in CSV_COLUMNS] for d in rows))


def run_importance(model: str, argv, log=print) -> dict:
    def add_arguments(ap):
        ap.add_argument("--repeats", type=int, default=5, help="shuffles per column (default 5)")
        ap.add_argument("--columns", default=None, help="comma-separated input columns (default: all)")

    ns, cfg, schema, out_path, load_predictor, load_data = scoring_job(
        "importance", "importance", "importance", "dataPath (the data: held-out rows)", model, argv, add_arguments)
    if skipped := other_rank(model, out_path):
        return skipped
    job = PermutationImportance(load_predictor(), repeats=ns.repeats, seed=cfg.seed)
    table = load_data()
    result = job.run(table, columns=comma_list(ns.columns), target=cfg.target)
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
