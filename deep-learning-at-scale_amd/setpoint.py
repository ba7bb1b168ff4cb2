"""Set points: at which value of ONE input column does a saved model predict the wanted value, row by row?

    python -m wellflow.setpoint <model> columnNames columnTypes targetColumn storagePath dataPath
                                --column C (--want V | --want-column COL) [--grid v1,v2,..] [--points P=17]
                                [--refine S=12] [--out PATH]
                                [--device D] [--precision P] [--seq-len T] [--group-col COL] [--batch-size B] [--header]

The inverse of ``predict``: every row keeps its own values in all columns but one, and that one is
searched for the value at which the prediction meets the row's wanted value. "This well, at today's
pressure and GLR: what choke opening gives the flow I want?" is what Gilbert's equation was written
for (``q = P S^C / (A R^B)``, so ``S* = (q A R^B / P)^(1/C)``), and ``gilbert`` over ``choke`` is
the closed form a learned answer is read against. ``--want-column`` may be the target column
itself: "which choke would have given the measured flow", a consistency check against the recorded
choke. Only a continuous column can be searched.

A run is ``1 + G + S`` scoring passes (scoring.py): the table as it is (the echoed ``prediction``),
G scan passes in which the column is one grid value in every row (``--grid`` floats kept as float32
in the order given, or ``--points`` values from the column's minimum to its maximum by
``np.linspace`` in float64 cast to float32), then S refine passes in which every bracketed row is
scored at the midpoint of its own bracket.

The rule, per prediction i. ``p``: the fp32 network output of the pass; ``want[i]``: the fp32
wanted value in raw target units; ``x``: the fp32 raw value the column had for this row in this
pass. The residual is formed in float64 and never contracted:

    r = (double)p * y_scale + y_shift - (double)want[i]

State: ``lo, hi, best_x, xq`` fp32; ``f_lo, f_hi, best_r`` fp64; ``status`` int32 (0 open,
1 bracketed).

* Scan pass g (``x = grid[g]``, the same for all rows; the grid is scanned in the order given).
  g == 0: ``status = 0; lo = hi = best_x = x; f_lo = f_hi = best_r = r``. g > 0, rows with
  ``status == 0``, in this order: if ``fabs(r) < fabs(best_r)`` or (``best_r`` is NaN and ``r`` is
  not) then ``best_x = x, best_r = r`` (a strict ``<``: the first of equal misses wins); if
  ``(f_lo <= 0 && r >= 0) || (f_lo >= 0 && r <= 0)`` then ``hi = x; f_hi = r; status = 1`` (``lo,
  f_lo`` remain the previous grid point); otherwise ``lo = hi = x; f_lo = f_hi = r``. Rows with
  ``status == 1`` are left alone: the first crossing in grid order wins. A NaN never brackets.
* Refine pass (``x = xq[i]``, the value this row was scored at), rows with ``status == 1``:
  ``same = f_lo < 0 ? r < 0 : (f_lo > 0 ? r > 0 : false)``; if ``same`` then ``lo = x, f_lo = r``,
  otherwise ``hi = x, f_hi = r``. Rows with ``status == 0`` are left alone.
* End of every pass: ``xq[i] = status == 1 ? lo + (hi - lo) * 0.5f : best_x``, in fp32.
* Finish, on the host in float64, after the one read of the state. Bracketed rows:
  ``setpoint = lo + (hi - lo) * (f_lo / (f_lo - f_hi))``, or ``lo`` when ``f_lo == f_hi``;
  ``miss = max(|f_lo|, |f_hi|)``. Open rows: ``setpoint = best_x``, status ``nearest``,
  ``miss = best_r``. A NaN residual reaches its own row only; a row whose miss is NaN shows ``nan``.

Routes. On the native path (GPU, bf16) nothing leaves the device between the first pass and the
last: the grid is uploaded once and element g serves both the assembly kernel's constant column
(csrc/features.hip) and the rule (csrc/score.hip solve_step); a refine pass hands the state's ``xq``
row to the assembly kernel as the column's per-row values (``perm_values``, read through an
identity index vector uploaded once, so a piece of the table gathers from the whole vector); the
state is read once at the end. An MLP table in pieces takes the same route. A table wider than the
device assembly's limit is assembled on the host and scored by the native engine: solve_step still
runs on the device and ``xq`` comes back to the host once per refine pass (announced once). On the
CPU / in fp32 the numpy rule (:func:`solve_step_host`) runs on the oracle's predictions: that path
is the oracle of the native one. ``gilbert`` runs the same rule in host float64 over whp, choke
and glr. The LSTM runs the scan only: overlapping windows share rows of the row table, so a
per-window value has no row to live in; ``--refine`` is set to 0 for it, with one notice on
stderr. ``want`` is taken at each window's last row.
"""
from __future__ import annotations

import sys

import numpy as np
import torch

from .predict import Predictor, _numeric_target, scoring_job
from .scoring import ConstantColumn, RowValues
from .whatif import comma_list, input_columns, other_rank, scorer_for, select_columns, table_rows, write_csv

NO_COLUMN = "no column to search: name it (--column C)"
RESULT_COLUMNS = ("prediction", "wanted", "setpoint", "status", "lo", "hi", "miss")
STATUS_NAMES = ("nearest", "bracketed", "nan")
FIRST, SCAN, REFINE = 0, 1, 2  # ops/native.py SOLVE_FIRST / SOLVE_SCAN / SOLVE_REFINE


# ---------------------------------------------------------------------- the rule, in numpy
def new_state(M: int) -> tuple:
    """(xs float32 [4][M]: lo, hi, best_x, xq; fs float64 [3][M]: f_lo, f_hi, best_r; status int32 [M])."""
    return np.zeros((4, M), np.float32), np.zeros((3, M), np.float64), np.zeros(M, np.int32)


def solve_step_host(p, want, y_scale: float, y_shift: float, mode: int, grid_x, xs, fs, status) -> None:
    """One pass of the rule on the host, in place (what csrc/score.hip solve_step computes on the
    device): ``p`` the pass's predictions [M] (fp32 network outputs; gilbert's float64 flows are
    used as they are), ``want`` float32 [M], ``grid_x`` the pass's value (scan modes)."""
    lo, hi, bx, xq = xs
    flo, fhi, br = fs
    r = np.asarray(p).astype(np.float64) * float(y_scale) + float(y_shift) - np.asarray(want, np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        if mode == FIRST:
            x = np.float32(grid_x)
            status[:] = 0
            lo[:], hi[:], bx[:] = x, x, x
            flo[:], fhi[:], br[:] = r, r, r
        elif mode == SCAN:
            x = np.float32(grid_x)
            opn = status == 0
            better = opn & ((np.abs(r) < np.abs(br)) | (np.isnan(br) & ~np.isnan(r)))
            cross = opn & (((flo <= 0) & (r >= 0)) | ((flo >= 0) & (r <= 0)))
            move = opn & ~cross
            bx[better], br[better] = x, r[better]
            hi[cross], fhi[cross], status[cross] = x, r[cross], 1
            lo[move], hi[move] = x, x
            flo[move], fhi[move] = r[move], r[move]
        elif mode == REFINE:
            x = xq.copy()
            same = np.where(flo < 0, r < 0, np.where(flo > 0, r > 0, False))
            near, far = (status == 1) & same, (status == 1) & ~same
            lo[near], flo[near] = x[near], r[near]
            hi[far], fhi[far] = x[far], r[far]
        else:
            raise ValueError(f"solve_step: mode {mode} is not 0 (first scan), 1 (scan) or 2 (refine)")
        xq[:] = np.where(status == 1, lo + (hi - lo) * np.float32(0.5), bx)


def finish_host(xs, fs, status) -> dict:
    """The answer of every row from the final state, in float64."""
    lo, hi, bx = (np.asarray(v, np.float64) for v in xs[:3])
    flo, fhi, br = (np.asarray(v, np.float64) for v in fs)
    got = np.asarray(status) == 1
    with np.errstate(all="ignore"):
        secant = np.where(flo == fhi, lo, lo + (hi - lo) * (flo / (flo - fhi)))
        setpoint = np.where(got, secant, bx)
        miss = np.where(got, np.maximum(np.abs(flo), np.abs(fhi)), br)
    code = np.where(np.isnan(miss), 2, np.where(got, 1, 0)).astype(np.int64)
    return {"setpoint": setpoint, "miss": miss, "code": code, "lo": lo, "hi": hi, "f_lo": flo, "f_hi": fhi,
            "best_x": bx, "best_r": br, "xq": np.asarray(xs[3], np.float32).copy(),
            "bracket": np.asarray(status, np.int32).copy()}


# ---------------------------------------------------------------------- the job's library form
class SetPoint:
    """``SetPoint(predictor, points=17, refine=12, piece_rows=0).run(table, column, want, grid=None)``.

    ``column``: the continuous input column to search. ``want``: the wanted prediction in raw
    target units, a scalar or one value per table row (for the LSTM it is taken at each window's
    last row). ``grid``: the scan values (kept as float32, in the order given) instead of
    ``points`` evenly spaced values from the column's minimum to its maximum. ``refine``: the
    number of midpoint passes after the scan. ``piece_rows``: rows of the assembled MLP table per
    piece on the native path (scoring.py)."""

    def __init__(self, predictor: Predictor, points: int = 17, refine: int = 12, piece_rows: int = 0, note=None):
        if predictor.name == "cnn":
            raise ValueError("set points do not apply to cnn: the CNN reads only the target's own history, so "
                             "there is no input column to search")
        if int(points) < 2:
            raise ValueError(f"points must be >= 2 (a scan from the column's minimum to its maximum), got {points}")
        if int(refine) < 0:
            raise ValueError(f"refine must be >= 0 (the midpoint passes after the scan), got {refine}")
        self.pred, self.points, self.refine, self.piece_rows = predictor, int(points), int(refine), int(piece_rows)
        self.note = note if note is not None else (lambda s: print(s, file=sys.stderr))

    def input_columns(self) -> list:
        """[(name, kind)] in the assembly kernel's source order (categorical, then continuous)."""
        return input_columns(self.pred)

    def _grid(self, table: dict, name: str, values) -> np.ndarray:
        if values is None:
            col = np.asarray(table[name], np.float32)
            return np.linspace(float(col.min()), float(col.max()), self.points, dtype=np.float64).astype(np.float32)
        g = []
        for v in values:
            try:
                g.append(float(v))
            except (TypeError, ValueError):
                raise ValueError(f"grid value {v!r} of the column {name!r} is not a number") from None
        if len(g) < 2:
            raise ValueError(f"the grid of column {name!r} holds {len(g)} value(s): a scan needs at least 2")
        return np.asarray(g, np.float64).astype(np.float32)

    def _want(self, want, n: int, rows) -> np.ndarray:
        w = np.asarray(want)
        if w.dtype.kind not in "fiu":
            raise ValueError(f"the wanted values must be numbers, got {w.dtype}")
        if w.ndim == 0:
            return np.full(n if rows is None else len(rows), w, np.float32)
        if w.shape != (n,):
            raise ValueError(f"want must be a scalar or one value per row ([{n}]), got {tuple(w.shape)}")
        w = w.astype(np.float32)
        return np.ascontiguousarray(w if rows is None else w[rows])

    def run(self, table: dict, column: str, want, grid=None) -> dict:
        pred = self.pred
        if isinstance(column, (list, tuple)):
            raise ValueError(f"ONE column is searched, got {list(column)}")
        k = select_columns(pred, [column] if column else [], NO_COLUMN, default_all=False,
                           target="a set point is searched over an INPUT column")[0]
        name, kind = self.input_columns()[k]
        if kind != "continuous":
            raise ValueError(f"column {name!r} is categorical: a bracket search needs a continuous column "
                             f"(sweep its labels with the response job)")
        n = table_rows(pred, table)
        grid = self._grid(table, name, grid)
        refine = self.refine
        if pred.name == "lstm" and refine > 0:
            self.note("setpoint: the LSTM runs the scan only (overlapping windows share rows of the row table, so a "
                      "per-window value has no row to live in): --refine is set to 0")
            refine = 0
        scorer = scorer_for(pred, table, "set-point", self.piece_rows)
        search = BracketSearch(scorer, k, self._want(want, n, scorer.rows), self.note)
        with torch.no_grad():
            search.baseline()
            for g, edit in enumerate(search.constants(grid)):
                search.scan(g, edit)
            for _ in range(refine):
                search.refine()
        xs, fs, status, p0 = search.finish()  # the one read of the device
        res = finish_host(xs, fs, status)
        code = res["code"]
        width = np.abs(res["hi"] - res["lo"])[res["bracket"] == 1]
        res.update({
            "model": pred.name, "native": bool(scorer.native), "n": n, "scored": int(scorer.M), "column": name,
            "grid": grid, "refine": refine, "passes": 1 + len(grid) + refine,
            "rows": np.arange(n) if scorer.rows is None else np.asarray(scorer.rows),
            "prediction": np.asarray(p0).astype(np.float64) * scorer.y_scale + scorer.y_shift,
            "wanted": search.want.astype(np.float64), "status": [STATUS_NAMES[c] for c in code],
            "bracketed": int((res["bracket"] == 1).sum()), "open": int((res["bracket"] != 1).sum()),
            "median_width": float(np.median(width)) if len(width) else float("nan")})
        return res


# ---------------------------------------------------------------------- the reduction
class BracketSearch:
    """Every pass of the scorer (whatif.py) moves the per-row state by the rule: on the device
    (csrc/score.hip solve_step) when the NATIVE engine scored (the predictions are there, whichever
    side assembled), else :func:`solve_step_host`. ``k``: the searched source column; ``want``:
    float32 [M], one wanted value per prediction."""

    def __init__(self, scorer, k: int, want: np.ndarray, note=None):
        self.scorer, self.k, self.want, self.device = scorer, int(k), want, scorer.native
        M = scorer.M
        if self.device:
            dev = scorer.pred.device
            self.xs = torch.zeros((4, M), dtype=torch.float32, device=dev)
            self.fs = torch.zeros((3, M), dtype=torch.float64, device=dev)
            self.status = torch.zeros(M, dtype=torch.int32, device=dev)
            self.want_dev = torch.from_numpy(want).to(dev)
            # rows [a, b) of a piece read the per-row values through ident[a:b]: one upload
            self.ident = torch.arange(M, dtype=torch.int32, device=dev) if scorer.on_device else None
            if not scorer.on_device and note is not None:
                note("setpoint: the table is assembled on the host: the rule still runs on the device and xq comes "
                     "back to the host once per refine pass")
        else:
            self.xs, self.fs, self.status = new_state(M)

    def constants(self, grid: np.ndarray) -> list:
        """The edits of the scan; on the device element g of ONE upload of the grid serves both
        the assembly kernel and the rule."""
        if not self.device:
            self.grid = grid
            return [ConstantColumn(self.k, h) for h in grid]
        self.grid = torch.from_numpy(np.ascontiguousarray(grid, np.float32)).to(self.scorer.pred.device)
        on = self.scorer.on_device
        return [ConstantColumn(self.k, h, self.grid[g : g + 1] if on else None) for g, h in enumerate(grid)]

    def baseline(self) -> None:
        p = self.scorer.predict()  # kept (a copy): the echoed prediction
        self.p0 = p.clone() if self.device else np.array(p, copy=True)

    def step(self, p, mode: int, g: int = -1) -> None:
        s = self.scorer
        if self.device:
            from .ops.native import solve_step

            solve_step(p, self.want_dev, s.y_scale, s.y_shift, mode, self.grid[g : g + 1] if mode != REFINE else None,
                       self.xs, self.fs, self.status)
        else:
            solve_step_host(p, self.want, s.y_scale, s.y_shift, mode, self.grid[g] if mode != REFINE else None,
                            self.xs, self.fs, self.status)

    def scan(self, g: int, edit) -> None:
        self.step(self.scorer.predict(edit), FIRST if g == 0 else SCAN, g)

    def refine(self) -> None:
        edit = RowValues(self.k, self.xs[3], self.ident) if self.device else RowValues(self.k, self.xs[3].copy())
        self.step(self.scorer.predict(edit), REFINE)

    def finish(self):
        self.scorer.check_device_errors()
        if self.device:
            return self.xs.cpu().numpy(), self.fs.cpu().numpy(), self.status.cpu().numpy(), self.p0.cpu().numpy()
        return self.xs, self.fs, self.status, np.asarray(self.p0)


# ---------------------------------------------------------------------- the job
def _write_csv(path: str, table: dict, names: list, result: dict) -> None:
    """The parsed table's columns, echoed, then prediction, wanted, setpoint, status, lo, hi and
    miss; a row without a prediction (the first T - 1 rows of an LSTM series) gets empty cells.
    Always with a header; floats as ``repr``. Atomic (tmp + rename)."""
    n = result["n"]
    pos = np.full(n, -1, np.int64)
    pos[result["rows"]] = np.arange(len(result["rows"]))
    echo = [np.asarray(table[c]).astype(str) for c in names]

    def cells(m):
        if m < 0:
            return [""] * len(RESULT_COLUMNS)
        return [result[c][m] if c == "status" else repr(float(result[c][m])) for c in RESULT_COLUMNS]

    write_csv(path, list(names) + list(RESULT_COLUMNS), ([e[i] for e in echo] + cells(m) for i, m in enumerate(pos)))


def run_setpoint(model: str, argv, log=print) -> dict:
    def add_arguments(ap):
        ap.add_argument("--column", default=None, help="the continuous input column to search")
        ap.add_argument("--want", default=None, help="the wanted prediction, one value for every row")
        ap.add_argument("--want-column", default=None, help="data column that holds every row's wanted prediction")
        ap.add_argument("--grid", default=None, help="comma-separated scan values, in the order given")
        ap.add_argument("--points", type=int, default=17, help="points of the default scan grid (default 17)")
        ap.add_argument("--refine", type=int, default=12, help="midpoint passes after the scan (default 12)")

    ns, cfg, schema, out_path, load_predictor, load_data = scoring_job(
        "setpoint", "set-point", "setpoint", "dataPath --column C (--want V | --want-column COL)", model, argv,
        add_arguments)
    if not (ns.column or "").strip():
        raise ValueError(NO_COLUMN)
    if (ns.want is None) == (ns.want_column is None):
        raise ValueError("name the wanted prediction once: --want V (one value for every row) or --want-column COL "
                         f"(a data column), {'not both' if ns.want is not None else 'neither was given'}")
    if ns.want is not None:
        try:
            want = float(ns.want)
        except ValueError:
            raise ValueError(f"--want {ns.want!r} is not a number") from None
    if skipped := other_rank(model, out_path):
        return skipped
    job = SetPoint(load_predictor(), points=ns.points, refine=ns.refine)
    table = load_data()
    if ns.want_column is not None:
        if ns.want_column not in table:
            raise ValueError(f"the data lacks the --want-column {ns.want_column!r}")
        want = _numeric_target(table, ns.want_column)
        if want is None:
            raise ValueError(f"the --want-column {ns.want_column!r} is not numeric")
    result = job.run(table, ns.column.strip(), want, grid=comma_list(ns.grid))
    result["out"] = out_path
    _write_csv(out_path, table, schema.names, result)
    log("Rows scored: %d" % result["scored"])
    log("Rows bracketed: %d" % result["bracketed"])
    log("Rows without a crossing: %d" % result["open"])
    log("Median bracket width: %f" % result["median_width"])
    return result


def main(argv=None) -> int:
    argv = list(sys.argv[1:] if argv is None else argv)
    if not argv or argv[0] in ("-h", "--help"):
        print(__doc__)
        return 0
    run_setpoint(argv[0], argv[1:])
    return 0


if __name__ == "__main__":
    sys.exit(main())
