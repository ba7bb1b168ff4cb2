"""Response curves: how does a saved model's prediction move when ONE input column is set to a value?

    python -m wellflow.response <model> columnNames columnTypes targetColumn storagePath dataPath
                                --columns a[,b..] [--grid v1,v2,..] [--points P=9] [--by COL] [--out PATH]
                                [--device D] [--precision P] [--seq-len T] [--group-col COL] [--batch-size B] [--header]

A partial-dependence curve, overall and per group: every row of the data keeps its own values in
all columns but one, that one is set to a grid value, the table is scored, and the mean prediction
(per ``--by`` group, a well say) is one point of the curve. The natural reading is next to the
physical model: ``gilbert`` is a choke performance curve, so the learned curve over ``choke`` per
well is compared with Gilbert's over the same grid. Each named column is swept on its own.

Grids. A continuous column takes ``--grid`` values (parsed as float, kept as float32, in the order
given) or ``--points`` values evenly spaced from the column's minimum to its maximum in the data
(``np.linspace`` in float64, cast to float32). A categorical column takes ``--grid`` labels (a
label unseen in training maps to the unknown index, as at training time, and is noted once on
stderr) or every label of the saved indexer, in indexer order. ``--grid`` names one column's
values, so it is refused with more than one column.

A run is ``1 + sum(grid sizes)`` scoring passes (scoring.py): pass 0 scores the table as it is (the
baseline), then one pass per (column, value). On the native path (GPU, bf16) the raw columns and
each column's grid are uploaded once and every pass stays on the device: the assembly kernel with
one source column read from a one-element device array (csrc/features.hip) -> the engine's forward
-> the grouped fp64 sums of that pass (csrc/score.hip group_sums) into its own slot. The host reads
the slots once, after the last pass. On the CPU / in fp32 the table column is replaced on the host
and the same sums are formed in numpy float64 (``np.bincount``): that path is the oracle of the
native one. For the LSTM the column is constant over every row of the row table, so over every
timestep of every window: a steady-state what-if; a window belongs to the group of its last row.

Sums of a pass, per group g, in raw target units and float64 (p: the network's output):
``v = p * y_scale + y_shift``; ``{n_g, sum v, sum v * v}``. A cell's mean is ``sum v / n``, its
standard deviation ``sqrt(max(0, sum v^2 / n - mean^2))``, its delta the mean minus the baseline
mean of the same group. The overall cell adds the groups' sums on the host, in group order.
"""
from __future__ import annotations

import math
import sys

import numpy as np
import torch

from .predict import Predictor, scoring_job
from .scoring import ConstantColumn
from .whatif import comma_list, input_columns, other_rank, scorer_for, select_columns, table_rows, write_csv

NO_COLUMN = "no column to sweep: name the columns (--columns a[,b..])"
CSV_COLUMNS = ("column", "kind", "value", "group", "rows", "mean_prediction", "std_prediction", "delta")


def group_sums_host(v64: np.ndarray, ids: np.ndarray, G: int) -> np.ndarray:
    """{n_g, sum v, sum v * v} float64 [G][3] in numpy (what csrc/score.hip computes on the device)."""
    out = np.empty((G, 3), np.float64)
    out[:, 0] = np.bincount(ids, minlength=G)
    out[:, 1] = np.bincount(ids, weights=v64, minlength=G)
    out[:, 2] = np.bincount(ids, weights=v64 * v64, minlength=G)
    return out


class ResponseCurves:
    """``ResponseCurves(predictor, points=9, piece_rows=0).run(table, columns, grids=None, by=None)``.

    ``columns``: the input columns to sweep, each on its own. ``grids``: ``{column: values}`` for
    the columns that do not take their default grid (``points`` evenly spaced values from the data's
    minimum to its maximum / every label the indexer knows). ``by``: a data column whose distinct
    values (as strings, sorted) are the groups; without it there is one group, the overall cell.
    ``piece_rows``: rows of the assembled MLP table per piece on the native path (scoring.py)."""

    def __init__(self, predictor: Predictor, points: int = 9, piece_rows: int = 0, note=None):
        if predictor.name == "cnn":
            raise ValueError("response curves do not apply to cnn: the CNN reads only the target's own "
                             "history, so there is no input column to set")
        if int(points) < 2:
            raise ValueError(f"points must be >= 2 (a curve from the column's minimum to its maximum), got {points}")
        self.pred, self.points, self.piece_rows = predictor, int(points), int(piece_rows)
        self.note = note if note is not None else (lambda s: print(s, file=sys.stderr))

    # ------------------------------------------------------------------ columns and grids
    def input_columns(self) -> list:
        """[(name, kind)] in the assembly kernel's source order (categorical, then continuous)."""
        return input_columns(self.pred)

    def _grid(self, table: dict, name: str, kind: str, values):
        """(values as written, host values, codes or None) of one column's grid."""
        if kind == "continuous":
            if values is None:
                col = np.asarray(table[name], np.float32)
                g = np.linspace(float(col.min()), float(col.max()), self.points, dtype=np.float64).astype(np.float32)
            else:
                g = []
                for v in values:
                    try:
                        g.append(float(v))
                    except (TypeError, ValueError):
                        raise ValueError(f"grid value {v!r} of the continuous column {name!r} is not a number") from None
                g = np.asarray(g, np.float64).astype(np.float32)
            if not len(g):
                raise ValueError(f"the grid of column {name!r} is empty")
            return [repr(float(v)) for v in g], list(g), None
        ix = next(ix for ix in self.pred.pipe.indexers if ix.column == name)
        labels = [str(v) for v in (ix.labels if values is None else values)]
        if not labels:
            raise ValueError(f"the grid of column {name!r} is empty")
        lut = {k: i for i, k in enumerate(ix.labels)}
        unseen = [v for v in labels if v not in lut]
        if unseen:
            self.note(f"response: column {name!r}: label(s) {unseen} were not seen in training; they map to the "
                      f"unknown index, as at training time")
        return labels, labels, np.asarray([lut.get(v, len(ix.labels)) for v in labels], np.int32)

    # ------------------------------------------------------------------ the run
    def run(self, table: dict, columns, grids=None, by: str | None = None) -> dict:
        pred = self.pred
        picked = select_columns(pred, columns, NO_COLUMN, default_all=False,
                                target="a response curve sets an INPUT column")
        have = self.input_columns()
        n = table_rows(pred, table)
        grids = dict(grids or {})
        for c in grids:
            if c not in [have[k][0] for k in picked]:
                raise ValueError(f"a grid is given for column {c!r}, which is not swept")
        if by is not None:
            if by not in table:
                raise ValueError(f"the data lacks the --by column {by!r}")
            groups, row_ids = np.unique(np.asarray(table[by]).astype(str), return_inverse=True)
            groups, row_ids = [str(g) for g in groups], row_ids.reshape(-1).astype(np.int64)
        else:
            groups, row_ids = [], np.zeros(n, np.int64)
        G = max(1, len(groups))
        from .ops.native import GROUP_SUMS_MAX_GROUPS

        if G > GROUP_SUMS_MAX_GROUPS:
            raise ValueError(f"--by {by!r} makes {G} groups; at most {GROUP_SUMS_MAX_GROUPS} are supported")
        plan = [(k, *self._grid(table, have[k][0], have[k][1], grids.get(have[k][0]))) for k in picked]
        scorer = scorer_for(pred, table, "response", self.piece_rows)
        grp = GroupSums(scorer, row_ids, G)
        grp.begin(1 + sum(len(shown) for _, shown, _, _ in plan))
        with torch.no_grad():
            grp.score(0)
            slot = 1
            for k, shown, host, codes in plan:
                for c in grp.constants(k, host, codes):  # one upload of the whole grid
                    grp.score(slot, c)
                    slot += 1
        sums = grp.finish()  # float64 [passes][G][3]: the one read of the device
        curves = []

        def cells(slot, column, kind, value):
            # overall first (the groups' sums added in group order), then the groups
            tot = np.cumsum(sums[slot], axis=0)[-1]
            rows = [("", tot, np.cumsum(sums[0], axis=0)[-1])]
            rows += [(g, sums[slot, i], sums[0, i]) for i, g in enumerate(groups)]
            for g, (cnt, s1, s2), (bn, b1, _) in rows:
                d = {"column": column, "kind": kind, "value": value, "group": g, "rows": int(cnt),
                     "mean_prediction": None, "std_prediction": None, "delta": None}
                if cnt > 0:
                    mean = s1 / cnt
                    d["mean_prediction"] = float(mean)
                    var = s2 / cnt - mean * mean
                    d["std_prediction"] = float(math.sqrt(max(0.0, var))) if var == var else float("nan")  # NaN is shown
                    d["delta"] = float(mean - b1 / bn)
                curves.append(d)

        cells(0, "", "baseline", "")
        slot = 1
        for k, shown, _, _ in plan:
            for v in shown:
                cells(slot, have[k][0], have[k][1], v)
                slot += 1
        return {"model": pred.name, "native": bool(scorer.native), "rows": n, "scored": int(scorer.M), "groups": groups,
                "by": by, "grids": {have[k][0]: list(shown) for k, shown, _, _ in plan}, "sums": sums, "curves": curves,
                "baseline_mean": curves[0]["mean_prediction"]}


# ---------------------------------------------------------------------- the reduction
class GroupSums:
    """``score(slot, edit)`` scores the edited table (whatif.py) and leaves the pass's grouped sums
    in ``slot``; ``finish()`` returns them all. The sums are formed on the device (csrc/score.hip)
    when the NATIVE engine scored (the predictions are there, whichever side assembled), else in
    numpy. A prediction belongs to its row (MLP) or to the last row of its window (LSTM)."""

    def __init__(self, scorer, row_ids: np.ndarray, G: int):
        self.scorer, self.G, self.device = scorer, G, scorer.native
        self.ids = row_ids if scorer.rows is None else row_ids[scorer.rows]
        if self.device:
            from .ops.native import GroupPlan

            self.plan = GroupPlan(self.ids, G, scorer.pred.device)

    def begin(self, passes: int) -> None:
        if self.device:
            self.out = torch.zeros((passes, self.G, 3), dtype=torch.float64, device=self.scorer.pred.device)
        else:
            self.sums = np.zeros((passes, self.G, 3), np.float64)

    def constants(self, k: int, host, codes) -> list:
        """The edits of one column's grid; the device assembly reads element g of one upload."""
        if not self.scorer.on_device:
            return [ConstantColumn(k, h) for h in host]
        grid = torch.from_numpy(codes if codes is not None else np.asarray(host, np.float32)).to(self.scorer.pred.device)
        return [ConstantColumn(k, h, grid[g : g + 1]) for g, h in enumerate(host)]

    def reduce(self, slot: int) -> None:
        from .ops.native import group_sums

        s = self.scorer
        group_sums(s.ps.p, self.plan, s.y_scale, s.y_shift, self.out, slot)

    def score(self, slot: int, edit=None) -> None:
        s = self.scorer
        p = s.predict(edit)
        if self.device:
            self.reduce(slot)
        else:
            v = np.asarray(p).astype(np.float64) * s.y_scale + s.y_shift
            self.sums[slot] = group_sums_host(v, self.ids, self.G)

    def finish(self) -> np.ndarray:
        self.scorer.check_device_errors()
        return self.out.cpu().numpy() if self.device else self.sums


# ---------------------------------------------------------------------- the job
def _write_csv(path: str, rows: list) -> None:
    """Baseline rows first, then column by column, value by value, overall then groups; always with
    a header; a cell without rows is left empty."""

    def cell(v):
        if v is None:
            return ""
        if isinstance(v, (str, int)):
            return str(v)
        return repr(float(v))

    write_csv(path, CSV_COLUMNS, ([cell(d[c]) for c in CSV_COLUMNS] for d in rows))


def run_response(model: str, argv, log=print) -> dict:
    def add_arguments(ap):
        ap.add_argument("--columns", default=None, help="comma-separated input columns to sweep, each on its own")
        ap.add_argument("--grid", default=None, help="comma-separated grid values (one column only)")
        ap.add_argument("--points", type=int, default=9, help="points of a default continuous grid (default 9)")
        ap.add_argument("--by", default=None, help="data column whose distinct values are the groups")

    ns, cfg, schema, out_path, load_predictor, load_data = scoring_job(
        "response", "response-curve", "response", "dataPath --columns a[,b..]", model, argv, add_arguments)
    columns = comma_list(ns.columns)
    if not columns:
        raise ValueError(NO_COLUMN)
    if ns.grid is not None and len(columns) > 1:
        raise ValueError(f"--grid gives ONE column's values; {len(columns)} columns are named (run them one by one)")
    if skipped := other_rank(model, out_path):
        return skipped
    job = ResponseCurves(load_predictor(), points=ns.points)
    table = load_data()
    grids = {columns[0]: comma_list(ns.grid)} if ns.grid is not None else None
    result = job.run(table, columns, grids=grids, by=ns.by)
    result["out"] = out_path
    _write_csv(out_path, result["curves"])
    log("Rows scored: %d" % result["scored"])
    log("Baseline mean prediction: %f" % result["baseline_mean"])
    for d in result["curves"]:
        if d["kind"] != "baseline" and d["group"] == "":
            log("%s = %s: mean prediction %f, delta %f" % (d["column"], d["value"], d["mean_prediction"], d["delta"]))
    return result


def main(argv=None) -> int:
    argv = list(sys.argv[1:] if argv is None else argv)
    if not argv or argv[0] in ("-h", "--help"):
        print(__doc__)
        return 0
    run_response(argv[0], argv[1:])
    return 0


if __name__ == "__main__":
    sys.exit(main())
