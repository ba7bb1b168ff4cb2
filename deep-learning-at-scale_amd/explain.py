"""Shapley attribution: which of the submitted columns moved THIS row's prediction, and by how much?

    python -m wellflow.explain <model> columnNames columnTypes targetColumn storagePath dataPath
                               [--repeats R=8] [--columns a,b,..] [--std] [--out PATH] [--seed S] [--device D]
                               [--precision P] [--seq-len T] [--group-col COL] [--batch-size B] [--header]

The prediction, importance and response jobs answer global questions. This one is local: per row
and per input column a contribution ``phi`` in raw target units which, added to a base value,
reproduces the row's prediction exactly (local accuracy). The raw column is what is attributed, so
a categorical column's whole one-hot block moves together.

The rule (sampling Shapley against background rows of the same table). ``K`` picked columns (all
input columns by default, always kept in the assembly kernel's source order: categorical, then
continuous), ``R`` repeats. Repeat ``r`` has a background row map ``perm_r [n]`` (row ``i`` is
paired with row ``perm_r[i]``) and a column order ``order_r`` (a permutation of the picked columns,
the same for all rows of the repeat).

* pass 0 scores the table as it is: ``p_full``;
* repeat ``r`` starts with ALL picked columns read through ``perm_r``: ``p_prev``; then, for
  ``j = 0 .. K-1``, column ``order_r[j]`` returns to the row's own value (columns ``order_r[j+1:]``
  still come from the background row) and the table is scored again: ``p_cur``. At ``j = K-1``
  nothing is left permuted, so ``p_cur`` is ``p_full`` and no pass is run: ``1 + R x K`` passes.

All arithmetic is float64 on the fp32 network outputs, never contracted: at the start of a repeat
``v = p_prev * y_scale + y_shift``, ``base += v``, ``base_sq += v * v``; at each step
``d = (p_cur - p_prev) * y_scale``, ``phi[k] += d``, ``sq[k] += d * d``, then ``p_prev = p_cur``.
At the end ``phi /= R``, ``base /= R`` and ``std = sqrt(max(0, sq / R - mean^2))``. Columns that
were not picked always keep the row's own value. With every one of the ``K!`` orders at one fixed
``perm`` ``phi`` is the exact Shapley value of the game ``v(S) = f(own values on S, background
values elsewhere)``; a column the model does not read, and an identity ``perm``, give exactly 0.0.

Draws. ``orders`` come from ``numpy.random.default_rng(seed)`` on the host (``R`` permutations of
``range(K)``, in repeat order). For mlp, mlp_online and gilbert the row maps come from
``torch.randperm`` on the scoring device, from a generator seeded with ``seed``, in repeat order
(as the importance job draws them). For the LSTM the map acts on the SERIES-SORTED row table and
is by default a cyclic shift ``perm_r[i] = (i + s_r) mod n`` with ``s_r`` in ``[1, n-1]`` drawn
from the host generator after the orders: a window's background is then another contiguous window,
not ``T`` unrelated rows. It may straddle a series boundary (the last rows of one series followed
by the first of the next). Both draws can be injected (``orders``, ``perms``).

On the native path (GPU, bf16) everything stays on the device: the raw columns and the column-set
masks of all passes are uploaded once; a pass is the assembly kernel's set launch
(csrc/features.hip: every column of the set read through the permutation) -> the engine's forward
-> ``attr_step`` (csrc/score.hip), which combines the pass with the previous one per row in the
fp64 tables. The tables are read once, after the last pass. On the CPU / in fp32 the same rule runs
in numpy float64 on host-permuted tables: that path is the oracle of the native one. ``gilbert``
is attributed over whp, choke and glr in host float64: Gilbert's equation is a product of powers of
the three, so a learned model's attributions have a physical counterpart to be read against.
"""
from __future__ import annotations

import sys

import numpy as np
import torch

from .predict import Predictor, _numeric_target, scoring_job
from .scoring import PermutedSet
from .whatif import Permutations, comma_list, input_columns, other_rank, scorer_for, select_columns, table_rows, write_csv


class ShapleyAttribution:
    """``ShapleyAttribution(predictor, repeats=8, seed=0, piece_rows=0).run(table, columns=None,
    orders=None, perms=None, target=None)``.

    ``columns``: the picked input columns (default: all); whatever order they are named in, they
    are kept in the assembly kernel's source order (:meth:`input_columns`), which is the order of
    ``result["columns"]`` and the order ``orders`` indexes. ``orders``: ints ``[R][K]``, each row a
    permutation of ``range(K)``. ``perms``: a tensor ``[R][n]`` or a callable ``r -> perm [n]``; n
    is the table's row count and, for the LSTM, the map acts on the series-sorted row table.
    ``piece_rows``: rows of the assembled MLP table per piece on the native path (scoring.py)."""

    def __init__(self, predictor: Predictor, repeats: int = 8, seed: int = 0, piece_rows: int = 0):
        if predictor.name == "cnn":
            raise ValueError("a Shapley attribution does not apply to cnn: the CNN reads only the target's own "
                             "history, so there is no input column to attribute a prediction to")
        if int(repeats) < 1:
            raise ValueError(f"repeats must be >= 1, got {repeats}")
        self.pred, self.repeats, self.seed, self.piece_rows = predictor, int(repeats), int(seed), int(piece_rows)

    def input_columns(self) -> list:
        """[(name, kind)] in the assembly kernel's source order (categorical, then continuous)."""
        return input_columns(self.pred)

    def _orders(self, orders, rng, R: int, K: int) -> np.ndarray:
        if orders is None:
            return np.stack([rng.permutation(K) for _ in range(R)]).astype(np.int64)
        o = np.asarray(orders)
        if o.dtype.kind not in "iu":
            raise TypeError(f"orders must be integers [{R}][{K}], got {o.dtype}")
        if o.shape != (R, K):
            raise ValueError(f"orders must be [{R}][{K}] (repeats, picked columns), got {tuple(o.shape)}")
        for r in range(R):
            if sorted(o[r].tolist()) != list(range(K)):
                raise ValueError(f"orders[{r}] = {o[r].tolist()} is not a permutation of 0 .. {K - 1}")
        return o.astype(np.int64)

    def run(self, table: dict, columns=None, orders=None, perms=None, target: str | None = None) -> dict:
        """``target``: the target column's name (gilbert only, and only for the reported MSE; a
        learned model's saved pipeline knows its own). The target column is not required."""
        pred = self.pred
        picked = sorted(select_columns(pred, columns, "no column to permute"))  # source order
        have = self.input_columns()
        n = table_rows(pred, table)
        R, K = self.repeats, len(picked)
        rng = np.random.default_rng(self.seed)
        orders = self._orders(orders, rng, R, K)
        cyclic = perms is None and pred.name == "lstm"
        perms = Permutations(perms, (R, n), "repeats, rows", "repeat")
        scorer = scorer_for(pred, table, "attribution", self.piece_rows)
        if cyclic:
            shifts = rng.integers(1, n, size=R) if n > 1 else np.zeros(R, np.int64)
        else:
            perms.bind(scorer, self.seed)
        # the column set of every pass that has one, repeat by repeat: all picked columns at the
        # start, then what is still permuted after step j (nothing after the last: that is p_full)
        sets = []
        for r in range(R):
            sets.append([picked[k] for k in orders[r]])
            sets += [[picked[k] for k in orders[r, j + 1:]] for j in range(K - 1)]
        att = Attribution(scorer)
        sets = att.column_sets(sets, len(have))
        att.begin(K)
        with torch.no_grad():
            att.full()
            for r in range(R):
                if cyclic:
                    perm = scorer.own_perms(torch.from_numpy((np.arange(n, dtype=np.int64) + int(shifts[r])) % n))
                else:
                    perm = perms.draw((r,), (r,))
                att.step(sets[r * K], perm, K, True)
                for j in range(K - 1):
                    att.step(sets[r * K + 1 + j], perm, int(orders[r, j]), False)
                att.last(int(orders[r, K - 1]))
        acc, sq, p_full = att.finish()  # float64 [K + 1][M] twice: the one read of the device
        mean = acc / R
        std = np.sqrt(np.maximum(0.0, sq / R - mean * mean))  # np.maximum keeps a NaN: shown, not hidden
        prediction = p_full.astype(np.float64) * scorer.y_scale + scorer.y_shift
        rows = np.arange(n) if scorer.rows is None else np.asarray(scorer.rows)
        result = {"model": pred.name, "native": bool(scorer.native), "n": n, "scored": int(scorer.M), "repeats": R,
                  "columns": [have[k][0] for k in picked], "orders": orders, "rows": rows,
                  "phi": mean[:K], "std": std[:K], "base": mean[K], "base_std": std[K], "prediction": prediction,
                  "acc": acc, "sq": sq, "mean_abs": np.abs(mean[:K]).mean(axis=1), "mse": None}
        tgt = pred.pipe.target if pred.pipe is not None else target
        y = _numeric_target(table, tgt) if tgt else None
        if y is not None:
            d = prediction - y[rows]
            result["mse"] = float(np.mean(d * d))
        return result


# ---------------------------------------------------------------------- the reduction
class Attribution:
    """Two consecutive passes of the scorer (whatif.py) are combined per row in the float64 tables
    ``acc`` / ``sq`` ``[K + 1][M]`` (row K: the base): on the device (csrc/score.hip attr_step)
    when the NATIVE engine scored (the predictions are there, whichever side assembled), else the
    same rule in numpy float64."""

    def __init__(self, scorer):
        self.scorer, self.device = scorer, scorer.native

    def column_sets(self, sets: list, n_sources: int) -> list:
        """(host, dev) of every set: the indices and, for the device assembly, the row of ONE
        upload of all masks ``[passes][words]`` that the pass points at."""
        if not self.scorer.on_device:
            return [(tuple(s), None) for s in sets]
        from .ops.native import column_masks

        masks = column_masks(sets, n_sources, self.scorer.pred.device)
        return [(tuple(s), masks[i]) for i, s in enumerate(sets)]

    def begin(self, K: int) -> None:
        M = self.scorer.M
        if self.device:
            dev = self.scorer.pred.device
            self.acc = torch.zeros((K + 1, M), dtype=torch.float64, device=dev)
            self.sq = torch.zeros((K + 1, M), dtype=torch.float64, device=dev)
            self.p_prev = torch.zeros(M, dtype=torch.float32, device=dev)
        else:
            self.acc = np.zeros((K + 1, M), np.float64)
            self.sq = np.zeros((K + 1, M), np.float64)

    def full(self) -> None:
        p = self.scorer.predict()  # kept (a copy): the last step of every repeat reads it
        self.p_full = p.clone() if self.device else np.array(p, copy=True)

    def accumulate(self, p, row: int, start: bool) -> None:
        s = self.scorer
        if self.device:
            from .ops.native import attr_step

            attr_step(p, self.p_prev, s.y_scale, s.y_shift, self.acc, self.sq, row, start)
        else:
            pc = np.asarray(p).astype(np.float64)
            d = pc * s.y_scale + s.y_shift if start else (pc - self.p_prev) * s.y_scale
            self.acc[row] += d
            self.sq[row] += d * d
            self.p_prev = pc

    def step(self, cols: tuple, perm, row: int, start: bool) -> None:
        self.accumulate(self.scorer.predict(PermutedSet(*cols, perm)), row, start)

    def last(self, row: int) -> None:
        self.accumulate(self.p_full, row, False)

    def finish(self):
        self.scorer.check_device_errors()
        if self.device:
            return self.acc.cpu().numpy(), self.sq.cpu().numpy(), self.p_full.cpu().numpy()
        return self.acc, self.sq, np.asarray(self.p_full)


# ---------------------------------------------------------------------- the job
def _write_csv(path: str, table: dict, names: list, result: dict, with_std: bool) -> None:
    """The parsed table's columns, echoed, then prediction, base, phi_<column> per picked column
    (source order) and, with ``with_std``, std_<column>; a row without a prediction (the first
    T - 1 rows of an LSTM series) gets empty cells. Always with a header; floats as ``repr``.
    Atomic (tmp + rename)."""
    n, cols = result["n"], result["columns"]
    blocks = [("prediction", result["prediction"]), ("base", result["base"])]
    blocks += [(f"phi_{c}", result["phi"][k]) for k, c in enumerate(cols)]
    if with_std:
        blocks += [(f"std_{c}", result["std"][k]) for k, c in enumerate(cols)]
    pos = np.full(n, -1, np.int64)
    pos[result["rows"]] = np.arange(len(result["rows"]))
    echo = [np.asarray(table[c]).astype(str) for c in names]
    write_csv(path, list(names) + [b for b, _ in blocks],
              ([e[i] for e in echo] + [repr(float(v[m])) if m >= 0 else "" for _, v in blocks] for i, m in enumerate(pos)))


def run_explain(model: str, argv, log=print) -> dict:
    def add_arguments(ap):
        ap.add_argument("--repeats", type=int, default=8, help="sampled column orders / background rows per row (default 8)")
        ap.add_argument("--columns", default=None, help="comma-separated input columns to attribute to (default: all)")
        ap.add_argument("--std", action="store_true", help="also write std_<column>: the spread over the repeats")

    ns, cfg, schema, out_path, load_predictor, load_data = scoring_job(
        "explain", "attribution", "explain", "dataPath", model, argv, add_arguments)
    if skipped := other_rank(model, out_path):
        return skipped
    job = ShapleyAttribution(load_predictor(), repeats=ns.repeats, seed=cfg.seed)
    table = load_data()
    result = job.run(table, columns=comma_list(ns.columns), target=cfg.target)
    result["out"] = out_path
    _write_csv(out_path, table, schema.names, result, ns.std)
    log("Rows scored: %d" % result["scored"])
    log("Rows without prediction: %d" % (result["n"] - result["scored"]))
    log("Mean prediction: %f" % float(np.mean(result["prediction"])))
    if result["mse"] is not None:
        log("Scoring MSE: %f" % result["mse"])
    by = sorted(range(len(result["columns"])), key=lambda k: (0, 0.0) if np.isnan(result["mean_abs"][k])
                else (1, -result["mean_abs"][k]))  # descending; NaN first (shown, not hidden); ties keep the order
    for k in by:
        log("%s: mean |phi| %f" % (result["columns"][k], result["mean_abs"][k]))
    return result


def main(argv=None) -> int:
    argv = list(sys.argv[1:] if argv is None else argv)
    if not argv or argv[0] in ("-h", "--help"):
        print(__doc__)
        return 0
    run_explain(argv[0], argv[1:])
    return 0


if __name__ == "__main__":
    sys.exit(main())
