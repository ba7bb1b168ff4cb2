"""Prediction intervals: "this well will flow 412" -- plus or minus what?

    python -m wellflow.interval <model> columnNames columnTypes targetColumn storagePath dataPath
                                [--calibrate] [--alpha 0.1[,0.05..]] [--by COL] [--relative] [--bands PATH] [--out PATH]
                                [--device D] [--precision P] [--seq-len T] [--group-col COL] [--batch-size B] [--header]

Split conformal prediction, per group ("Mondrian"), with the finite-sample rank. Two runs:

``--calibrate``: ``dataPath`` holds HELD-OUT rows with their target. They are scored once, every
prediction gets a score (its absolute residual; with ``--relative`` the residual as a share of the
prediction), and per ``--by`` group (a well, say) and per level ``alpha`` the
``ceil((n + 1) (1 - alpha))``-th smallest score of the group's ``n`` rows is the group's quantile ``q``:
the half-width of a band that covers at least ``1 - alpha`` of exchangeable rows. The quantiles go
into ``<storagePath>interval/<model>.bands.csv`` (``--bands``).

Without ``--calibrate`` the bands file is read (its ``by``, ``relative`` and levels hold; giving
them again is refused), ``dataPath`` is scored as the prediction job scores it, and
``<storagePath>interval/<model>.csv`` echoes the columns and adds ``prediction``, per level
``lower_<L>`` / ``upper_<L>`` (``L`` the coverage in percent, ``90`` for alpha 0.1) and ``band``
(``group``: the row's own group's quantile; ``overall``: the quantile of all calibration rows;
per level, joined by ``/``, when the levels differ).

The rule, per prediction (p: the fp32 network output, y: the fp32 raw target at the prediction's
row -- for the LSTM the last row of its window):
``v = p * y_scale + y_shift``, ``d = v - y`` in float64 (importance.py's ``d``);
``s = float32(|d|)``, with ``--relative`` ``float32(|d| / |v|)`` under IEEE rules (x / 0 is inf, 0 / 0
NaN). Gilbert's predictions are float64 in raw units already: ``d = p - y``, the same casts.
The groups are the distinct values of the ``--by`` column as strings, sorted; there is always an
overall group of all scored rows. For a group of ``n`` scored rows ``k1 = ceil((n + 1) (1 - alpha))``
in exact rational arithmetic from the decimal text of ``alpha``; ``k1 > n``: the group has no band
of its own at that level and takes the overall one (``source = overall``); the overall group
itself with ``k1 > n`` has the quantile ``+inf`` (said once on stderr). Else ``q = np.sort(s_g)[k1 -
1]`` (NaN sorts last; a NaN ``q`` is shown as ``nan`` and noted once on stderr).
Applied to a row with prediction ``v`` (the prediction job's value): ``half = q``, with ``--relative``
``q * |v|``; ``lower = v - half``, ``upper = v + half`` in float64. A row whose group the bands do not
know takes the overall band.

On a native engine (GPU, bf16) nothing leaves the device between the forward and the quantiles:
the scores are formed there (csrc/quantile.hip abs_scores) and the order statistics are selected
there, exactly (group_quantiles: a radix select over the scores' bit patterns, once over the
``--by`` plan and once over the one-group overall plan); the host reads the two small results. On
the CPU / in fp32 the numpy rule of this module runs on the oracle's predictions: it is the
oracle of the native path.
"""
from __future__ import annotations

import csv
import math
import os
import sys
from fractions import Fraction

import numpy as np
import torch

from .predict import Predictor, _numeric_target, scoring_job
from .whatif import comma_list, other_rank, scorer_for, table_rows, write_csv

BANDS_COLUMNS = ("by", "relative", "alpha", "group", "rows", "rank", "quantile", "source")
MAX_LEVELS = 4  # ops/native.py QUANTILE_MAX_LEVELS
NAN_KEY = 0x7FC00000
DEFAULT_ALPHA = "0.1"


# ---------------------------------------------------------------------- the rule
def parse_alphas(alphas) -> list:
    """The levels as their decimal texts, checked: at most ``MAX_LEVELS``, each in (0, 1), distinct."""
    texts = [str(a).strip() for a in ([alphas] if isinstance(alphas, (str, float)) else list(alphas))]
    if not 1 <= len(texts) <= MAX_LEVELS:
        raise ValueError(f"{len(texts)} levels: give 1 to {MAX_LEVELS} (--alpha 0.1[,0.05..])")
    seen = []
    for t in texts:
        try:
            f = Fraction(t)
        except (ValueError, ZeroDivisionError):
            raise ValueError(f"level {t!r} is not a decimal number") from None
        if not 0 < f < 1:
            raise ValueError(f"level {t!r} is outside (0, 1): alpha is the share of rows a band may miss")
        if f in seen:
            raise ValueError(f"level {t!r} is given twice")
        seen.append(f)
    return texts


def conformal_rank(n: int, alpha: str) -> int:
    """``k1 = ceil((n + 1) (1 - alpha))``, 1-based, in exact arithmetic from the text of ``alpha``."""
    return math.ceil((int(n) + 1) * (1 - Fraction(alpha)))


def level_name(alpha: str) -> str:
    """``90`` for alpha ``0.1``: the coverage in percent, as the CSV's column names carry it."""
    return "%g" % float(100 * (1 - Fraction(alpha)))


def score_host(p, y, y_scale: float = 1.0, y_shift: float = 0.0, relative: bool = False, learned: bool = True):
    """The scores float32 [M] in numpy (what csrc/quantile.hip abs_scores computes on the device).
    ``learned``: ``p`` are fp32 network outputs and ``y`` the fp32 raw target; else ``p`` are float64
    predictions in raw units (Gilbert) and ``y`` the float64 target."""
    if learned:
        v = np.asarray(p, np.float32).astype(np.float64) * float(y_scale) + float(y_shift)
        d = v - np.asarray(y, np.float32).astype(np.float64)
    else:
        v = np.asarray(p, np.float64)
        d = v - np.asarray(y, np.float64)
    with np.errstate(all="ignore"):
        s = np.abs(d) / np.abs(v) if relative else np.abs(d)
        return s.astype(np.float32)


def score_keys(s) -> np.ndarray:
    """The 32-bit patterns of the scores, every NaN as ``NAN_KEY``: for scores that are
    non-negative or NaN, unsigned key order is ``np.sort``'s order (NaN last)."""
    s = np.ascontiguousarray(s, np.float32)
    return np.where(np.isnan(s), np.uint32(NAN_KEY), s.view(np.uint32))


def select_host_radix(s, k: int) -> np.float32:
    """The ``k``-th smallest (0-based, clamped) score by the device's four-round byte select
    (csrc/quantile.hip), emulated in numpy: equals ``np.sort(s)[k]`` bit for bit. NaN without scores."""
    keys = score_keys(s).astype(np.int64)
    if not len(keys):
        return np.float32(np.nan)
    rank, prefix = min(max(int(k), 0), len(keys) - 1), 0
    for shift in (24, 16, 8, 0):
        live = keys[(keys >> (shift + 8)) == prefix]
        hist = np.bincount((live >> shift) & 255, minlength=256)
        run = np.cumsum(hist)
        b = int(np.argmax(run > rank))  # the first bin whose running count exceeds the rank
        rank -= int(run[b] - hist[b])
        prefix = (prefix << 8) | b
    return np.asarray([prefix], np.uint32).view(np.float32)[0]


def group_quantiles_host(s, ids, G: int, ranks) -> np.ndarray:
    """float32 [G][A]: per group the ``ranks[g][a]``-th smallest score (0-based, clamped into the
    group; NaN for an empty group) by ``np.sort`` (what the device op returns)."""
    s, ids, ranks = np.asarray(s, np.float32), np.asarray(ids), np.asarray(ranks)
    out = np.full(ranks.shape, np.nan, np.float32)
    order = np.argsort(ids, kind="stable")
    ends = np.searchsorted(ids[order], np.arange(G + 1))
    for g in range(G):
        sg = np.sort(s[order[ends[g] : ends[g + 1]]])
        if len(sg):
            out[g] = sg[np.clip(ranks[g], 0, len(sg) - 1)]
    return out


def select_ranks(counts, alphas) -> np.ndarray:
    """int32 [G][A], 0-based: ``k1 - 1`` where the group has its own band (``k1 <= n``), else 0 (the
    answer is not used)."""
    return np.asarray([[(k - 1 if k <= n else 0) for k in (conformal_rank(n, a) for a in alphas)] for n in counts],
                      np.int32).reshape(len(counts), len(alphas))


def make_bands(by, relative: bool, alphas, groups, counts, q_groups, n_all: int, q_all, note=None) -> dict:
    """The bands of a calibration: per level the overall row first, then the groups in order.
    ``q_groups`` float32 [G][A] / ``q_all`` float32 [A]: the selected quantiles (ignored where the
    rank rule gives none). A row: ``{alpha, group, rows, rank, quantile, source}``."""
    note = note if note is not None else (lambda s: print(s, file=sys.stderr))
    rows, said_inf, said_nan = [], False, False
    for a, alpha in enumerate(alphas):
        k1 = conformal_rank(n_all, alpha)
        q = float(q_all[a]) if k1 <= n_all else float("inf")
        if k1 > n_all and not said_inf:
            said_inf = True
            note(f"interval: {n_all} calibration rows are too few for alpha {alpha} (rank {k1}): the overall "
                 f"quantile is +inf, the band unbounded")
        rows.append({"alpha": alpha, "group": "", "rows": int(n_all), "rank": k1, "quantile": q, "source": "overall"})
        for g, name in enumerate(groups):
            n, kg = int(counts[g]), conformal_rank(int(counts[g]), alpha)
            own = kg <= n
            rows.append({"alpha": alpha, "group": name, "rows": n, "rank": kg,
                         "quantile": float(q_groups[g][a]) if own else q, "source": "group" if own else "overall"})
    for r in rows:
        if r["quantile"] != r["quantile"] and not said_nan:
            said_nan = True
            note(f"interval: a quantile is NaN (alpha {r['alpha']}, group {r['group']!r}): NaN scores (a NaN "
                 f"prediction or target, or 0 / 0 in relative mode) sort last and reached the rank")
    return {"by": by or "", "relative": bool(relative), "alphas": list(alphas), "groups": list(groups), "rows": rows}


# ---------------------------------------------------------------------- the bands file
def write_bands(path: str, bands: dict) -> None:
    """Always with a header; floats as ``repr`` (the round trip is exact). Atomic (tmp + rename)."""
    rel = "1" if bands["relative"] else "0"
    write_csv(path, BANDS_COLUMNS, ([bands["by"], rel, r["alpha"], r["group"], str(r["rows"]), str(r["rank"]),
                                     repr(float(r["quantile"])), r["source"]] for r in bands["rows"]))


def read_bands(path: str) -> dict:
    """The bands of :func:`write_bands`; a file that does not parse is refused with the reason."""
    if not os.path.exists(path):
        raise FileNotFoundError(f"no bands file at {path} (calibrate first: python -m wellflow.interval <model> ... "
                                f"--calibrate)")
    with open(path, newline="") as f:
        lines = list(csv.reader(f))
    bad = lambda why: ValueError(f"the bands file {path} does not parse: {why}")  # noqa: E731
    if not lines or tuple(lines[0]) != BANDS_COLUMNS:
        raise bad(f"its header is not {','.join(BANDS_COLUMNS)}")
    if len(lines) < 2:
        raise bad("it holds no band")
    rows, alphas, groups = [], [], []
    for i, c in enumerate(lines[1:], start=2):
        if len(c) != len(BANDS_COLUMNS):
            raise bad(f"line {i} has {len(c)} cells, not {len(BANDS_COLUMNS)}")
        if (c[0], c[1]) != (lines[1][0], lines[1][1]) or c[1] not in ("0", "1"):
            raise bad(f"line {i}: 'by' / 'relative' must be the same in every line, 'relative' 0 or 1")
        try:
            row = {"alpha": c[2].strip(), "group": c[3], "rows": int(c[4]), "rank": int(c[5]), "quantile": float(c[6]),
                   "source": c[7]}
            parse_alphas([row["alpha"]])
        except ValueError as e:
            raise bad(f"line {i}: {e}") from None
        if row["source"] not in ("group", "overall") or (row["group"] == "" and row["source"] != "overall"):
            raise bad(f"line {i}: source {row['source']!r} (group or overall; the overall row: overall)")
        if row["alpha"] not in alphas:
            if row["group"] != "":
                raise bad(f"line {i}: level {row['alpha']} does not begin with its overall row (an empty group cell)")
            alphas.append(row["alpha"])
        elif row["alpha"] != alphas[-1] or row["group"] == "":
            raise bad(f"line {i}: the rows of level {row['alpha']} are not together, or it has two overall rows")
        if row["group"] != "" and row["group"] not in groups:
            groups.append(row["group"])
        rows.append(row)
    try:
        parse_alphas(alphas)
    except ValueError as e:
        raise bad(str(e)) from None
    return {"by": lines[1][0], "relative": lines[1][1] == "1", "alphas": alphas, "groups": groups, "rows": rows}


# ---------------------------------------------------------------------- the job's two halves
class ConformalBands:
    """``ConformalBands(predictor, alphas=("0.1",), by=None, relative=False, piece_rows=0)``:
    ``.calibrate(table, target=None) -> bands`` scores held-out rows once and selects the quantiles;
    ``.apply(table, bands) -> result`` scores a table as the prediction job does and puts the bands
    around the predictions (the bands' own ``by``, ``relative`` and levels hold there).
    ``alphas``: the levels, as decimal texts; ``by``: a data column whose distinct values (as
    strings, sorted) are the groups; ``piece_rows``: rows of the assembled MLP table per piece on
    the native path (scoring.py)."""

    def __init__(self, predictor: Predictor, alphas=(DEFAULT_ALPHA,), by: str | None = None, relative: bool = False,
                 piece_rows: int = 0, note=None):
        if predictor.name == "cnn":
            raise ValueError("prediction intervals are not built for cnn: the CNN forecasts O horizons per window, "
                             "and a band per horizon is not built here")
        self.pred, self.alphas, self.by = predictor, parse_alphas(alphas), by or None
        self.relative, self.piece_rows = bool(relative), int(piece_rows)
        self.note = note if note is not None else (lambda s: print(s, file=sys.stderr))

    def _target(self, table: dict, target) -> np.ndarray:
        tgt = self.pred.pipe.target if self.pred.pipe is not None else target
        if not tgt:
            raise ValueError("gilbert: name the target column (calibrate(table, target=...))")
        if tgt not in table:
            raise ValueError(f"the data lacks the target column {tgt!r}: a calibration scores held-out rows against it")
        y = _numeric_target(table, tgt)
        if y is None:
            raise ValueError(f"the target column {tgt!r} is not numeric: a calibration needs a numeric target")
        return y

    @staticmethod
    def _groups(table: dict, by, n: int):
        if by is None:
            return [], np.zeros(n, np.int64)
        if by not in table:
            raise ValueError(f"the data lacks the --by column {by!r}")
        groups, ids = np.unique(np.asarray(table[by]).astype(str), return_inverse=True)
        return [str(g) for g in groups], ids.reshape(-1).astype(np.int64)

    # ------------------------------------------------------------------ calibrate
    def calibrate(self, table: dict, target: str | None = None) -> dict:
        """``target``: the target column's name (gilbert only; a learned model's saved pipeline knows
        its own). The result is the bands (:func:`make_bands`) plus ``scored`` / ``native``."""
        pred, A = self.pred, len(self.alphas)
        n = table_rows(pred, table)
        y = self._target(table, target)
        groups, row_ids = self._groups(table, self.by, n)
        G = len(groups)
        from .ops.native import QUANTILE_MAX_CELLS

        if G * A > QUANTILE_MAX_CELLS:
            raise ValueError(f"--by {self.by!r} makes {G} groups; with {A} level(s) at most {QUANTILE_MAX_CELLS // A} "
                             f"are supported")
        scorer = scorer_for(pred, table, "interval", self.piece_rows)
        ids = row_ids if scorer.rows is None else row_ids[scorer.rows]
        counts = np.bincount(ids, minlength=G) if G else np.zeros(0, np.int64)
        M = int(scorer.M)
        if scorer.learned:
            y = y.astype(np.float32)
            y = y if scorer.rows is None else y[scorer.rows]
        with torch.no_grad():
            p = scorer.predict()
        r_all, r_by = select_ranks([M], self.alphas), select_ranks(counts, self.alphas)
        if scorer.native:
            q_all, q_by = self._select_device(scorer, p, y, ids, G, r_all, r_by)
        else:
            s = score_host(np.asarray(p), y, scorer.y_scale, scorer.y_shift, self.relative, scorer.learned)
            q_all = group_quantiles_host(s, np.zeros(M, np.int64), 1, r_all)[0]
            q_by = group_quantiles_host(s, ids, G, r_by) if G else None
        bands = make_bands(self.by, self.relative, self.alphas, groups, counts, q_by, M, q_all, self.note)
        bands.update(model=pred.name, native=bool(scorer.native), scored=M, rows_in=n)
        return bands

    def _select_device(self, scorer, p, y32, ids, G: int, r_all, r_by):
        """abs_scores, then group_quantiles over the ``by`` plan and the one-group overall plan; one
        read of the two small results behind the engine's error check."""
        from .ops.native import QuantilePlan, abs_scores, group_quantiles

        dev, A, M = scorer.pred.device, len(self.alphas), int(scorer.M)
        s = torch.empty(M, dtype=torch.float32, device=dev)
        abs_scores(p, torch.from_numpy(np.ascontiguousarray(y32)).to(dev), scorer.y_scale, scorer.y_shift,
                   self.relative, s)
        outs = []
        for plan_ids, g, ranks in ((np.zeros(M, np.int64), 1, r_all), (ids, G, r_by)):
            if g < 1:
                outs.append(None)
                continue
            plan = QuantilePlan(plan_ids, g, A, dev)
            out = torch.empty((g, A), dtype=torch.float32, device=dev)
            group_quantiles(s, plan, torch.from_numpy(ranks).to(dev), out)
            outs.append(out)
        scorer.check_device_errors()
        return outs[0].cpu().numpy()[0], (outs[1].cpu().numpy() if outs[1] is not None else None)

    # ------------------------------------------------------------------ apply
    def apply(self, table: dict, bands: dict, target: str | None = None) -> dict:
        """``target``: the target column's name for the empirical coverage (gilbert only)."""
        pred = self.pred
        by, relative, alphas = bands["by"] or None, bool(bands["relative"]), list(bands["alphas"])
        if by is not None and by not in table:
            raise ValueError(f"the bands are per {by!r} (their 'by' column), which the data lacks")
        n = table_rows(pred, table)
        v = np.asarray(pred.predict_table(table))  # fp32 raw units (gilbert: float64); NaN: no prediction
        ok = ~np.isnan(v)
        v64 = v.astype(np.float64)
        names = np.asarray(table[by]).astype(str) if by is not None else None
        lower, upper, source = np.empty((len(alphas), n)), np.empty((len(alphas), n)), []
        for a, alpha in enumerate(alphas):
            rows = [r for r in bands["rows"] if r["alpha"] == alpha]
            q_all = rows[0]["quantile"]
            own = {r["group"]: r["quantile"] for r in rows[1:] if r["source"] == "group"}
            if names is None or not own:
                q, src = np.full(n, q_all, np.float64), np.zeros(n, bool)
            else:
                known = np.asarray(sorted(own))
                at = np.minimum(np.searchsorted(known, names), len(known) - 1)
                src = known[at] == names
                q = np.where(src, np.asarray([own[k] for k in known], np.float64)[at], q_all)
            with np.errstate(invalid="ignore"):
                half = q * np.abs(v64) if relative else q
                lower[a], upper[a] = v64 - half, v64 + half
            source.append(src)
        word = ("overall", "group")
        band = np.asarray([word[col[0]] if (col == col[0]).all() else "/".join(word[s] for s in col)
                           for col in np.asarray(source).T.astype(int)], dtype=object)
        result = {"model": pred.name, "native": bool(pred.native), "rows": n, "scored": int(ok.sum()),
                  "unscored": int(n - ok.sum()), "prediction": v, "lower": lower, "upper": upper, "band": band,
                  "has_prediction": ok, "alphas": alphas, "levels": [level_name(a) for a in alphas], "by": by,
                  "relative": relative, "coverage": None}
        tgt = pred.pipe.target if pred.pipe is not None else target
        y = _numeric_target(table, tgt) if tgt else None
        if y is not None and ok.any():
            result["coverage"] = [float(np.mean((lower[a][ok] <= y[ok]) & (y[ok] <= upper[a][ok])))
                                  for a in range(len(alphas))]
        return result


# ---------------------------------------------------------------------- the job
def _write_csv(path: str, table: dict, names: list, result: dict) -> None:
    """The parsed table's columns, echoed, then prediction, lower_<L> / upper_<L> per level and band;
    a row without a prediction gets empty cells. Always with a header; floats as ``repr``. Atomic."""
    echo = [np.asarray(table[c]).astype(str) for c in names]
    A = len(result["levels"])
    head = list(names) + ["prediction"] + [f"{side}_{L}" for L in result["levels"] for side in ("lower", "upper")] + ["band"]

    def cells(i):
        if not result["has_prediction"][i]:
            return [""] * (2 + 2 * A)
        out = [repr(float(result["prediction"][i]))]
        for a in range(A):
            out += [repr(float(result["lower"][a][i])), repr(float(result["upper"][a][i]))]
        return out + [result["band"][i]]

    write_csv(path, head, ([e[i] for e in echo] + cells(i) for i in range(result["rows"])))


def run_interval(model: str, argv, log=print) -> dict:
    def add_arguments(ap):
        ap.add_argument("--calibrate", action="store_true", help="score held-out rows and write the bands file")
        ap.add_argument("--alpha", default=None, help="comma-separated levels in (0, 1), at most 4 (default 0.1)")
        ap.add_argument("--by", default=None, help="data column whose distinct values are the groups")
        ap.add_argument("--relative", action="store_true", help="score the residual as a share of the prediction")
        ap.add_argument("--bands", default=None, help="bands CSV (default <storagePath>interval/<model>.bands.csv)")

    ns, cfg, schema, out_path, load_predictor, load_data = scoring_job(
        "interval", "interval", "interval", "dataPath [--calibrate]", model, argv, add_arguments)
    sp = cfg.storage_path
    if sp and not sp.endswith(("/", os.sep)):
        sp += os.sep
    bands_path = ns.bands or os.path.join(sp + "interval", f"{model}.bands.csv")
    if not ns.calibrate:
        given = [o for o, on in (("--alpha", ns.alpha is not None), ("--by", ns.by is not None),
                                 ("--relative", ns.relative)) if on]
        if given:
            raise ValueError(f"{', '.join(given)} given without --calibrate: the levels, the grouping and the mode "
                             f"are read from the bands file ({bands_path}); calibrate again to change them")
    alphas = parse_alphas(comma_list(ns.alpha) if ns.alpha is not None else [DEFAULT_ALPHA])
    if skipped := other_rank(model, bands_path if ns.calibrate else out_path):
        return skipped
    if ns.calibrate:
        job = ConformalBands(load_predictor(), alphas=alphas, by=ns.by, relative=ns.relative)
        bands = job.calibrate(load_data(), target=cfg.target)
        write_bands(bands_path, bands)
        bands["out"] = bands_path
        log("Calibration rows scored: %d" % bands["scored"])
        for r in bands["rows"]:
            if r["group"] == "":
                log("Overall quantile %s: %f" % (level_name(r["alpha"]), r["quantile"]))
        return bands
    bands = read_bands(bands_path)
    job = ConformalBands(load_predictor(), alphas=bands["alphas"])
    table = load_data()
    result = job.apply(table, bands, target=cfg.target)
    result["out"] = out_path
    _write_csv(out_path, table, schema.names, result)
    log("Rows scored: %d" % result["scored"])
    log("Rows without prediction: %d" % result["unscored"])
    for L, c in zip(result["levels"], result["coverage"] or ()):
        log("Empirical coverage %s: %f" % (L, c))
    return result


def main(argv=None) -> int:
    argv = list(sys.argv[1:] if argv is None else argv)
    if not argv or argv[0] in ("-h", "--help"):
        print(__doc__)
        return 0
    run_interval(argv[0], argv[1:])
    return 0


if __name__ == "__main__":
    sys.exit(main())
