"""What the what-if jobs share: the importance, response-curve and attribution jobs (importance.py,
response.py, explain.py) score ONE table again and again, each pass with its own edit
(scoring.py), and reduce every pass. Here: the input columns and the table checks, the scorer that
turns an edit into predictions (the physical model in host float64, or a pass of scoring.py), the
supply of permutations, and the tail of a job (the comma lists, rank 0, the atomic CSV). A job
adds its rule: the reduction of a pass, on the host and on the device, and the one condition that
picks between the two.
"""
from __future__ import annotations

import csv
import os

import numpy as np
import torch

from .models.gilbert import GilbertModel
from .scoring import LstmPass, MlpPass

GILBERT_INPUTS = ("whp", "choke", "glr")


# ---------------------------------------------------------------------- columns and table checks
def input_columns(pred) -> list:
    """[(name, kind)] of every input column, in the assembly kernel's source order: the
    categorical columns (saved indexer order), then the continuous ones."""
    if pred.name == "gilbert":
        return [(c, "continuous") for c in GILBERT_INPUTS]
    pipe = pred.pipe
    return [(ix.column, "categorical") for ix in pipe.indexers] + [(c, "continuous") for c in pipe.continuous]


def select_columns(pred, columns, none: str, default_all: bool = True, target: str | None = None) -> list:
    """The source indices of the named ``columns``, in the order given. ``default_all``: None
    picks every input column (else, as an empty list, it is refused with ``none``). ``target``:
    the job's reason why the target column is refused by name (else it is an unknown column)."""
    names = [c for c, _ in input_columns(pred)]
    if columns is None and default_all:
        return list(range(len(names)))
    picked = []
    for c in columns or ():
        if target and pred.pipe is not None and c == pred.pipe.target:
            raise ValueError(f"column {c!r} is the target column: {target}")
        if c not in names:
            what = ("gilbert reads only " + ", ".join(GILBERT_INPUTS)) if pred.name == "gilbert" else \
                f"the model's input columns are {names}"
            raise ValueError(f"unknown column {c!r}: {what}")
        if names.index(c) in picked:
            raise ValueError(f"column {c!r} listed twice")
        picked.append(names.index(c))
    if not picked:
        raise ValueError(none)
    return picked


def table_rows(pred, table: dict) -> int:
    """The table's row count; refused without rows or without one of the model's input columns."""
    n = len(next(iter(table.values()))) if table else 0
    if n < 1:
        raise ValueError("no rows to score")
    for c, _ in input_columns(pred):
        if c not in table:
            raise ValueError(f"the data lacks the input column {c!r}")
    return n


def target_scale(pipe) -> tuple:
    """(y_scale, y_shift): a network output p is ``p * y_scale + y_shift`` in raw target units."""
    return (float(pipe.y_std), float(pipe.y_mean)) if pipe.standardize_target else (1.0, 0.0)


# ---------------------------------------------------------------------- scorers
class Scorer:
    """One table, scored again and again: ``predict(edit)`` -> the ``M`` predictions of the table
    edited by ``edit`` (scoring.py; None: as it is). ``rows``: the table row of each prediction
    (None: every row, in order); ``perm_device`` / ``perm_dtype``: what a permutation must be."""

    learned = native = on_device = False
    rows = None
    perm_device = torch.device("cpu")
    perm_dtype = torch.int64
    y_scale, y_shift = 1.0, 0.0

    def own_perms(self, perms: torch.Tensor) -> torch.Tensor:
        return perms.to(self.perm_device, self.perm_dtype)

    def check_device_errors(self) -> None:
        pass


class GilbertScorer(Scorer):
    """The physical model in host float64 over whp, choke and glr: what a learned model's figures
    are read against. Its predictions are float64, in raw units, and are used as they are."""

    def __init__(self, pred, table: dict):
        self.model = GilbertModel(correlation=pred.extra.get("correlation", "gilbert"))
        self.cols = {k: np.asarray(table[k], np.float64) for k in GILBERT_INPUTS}
        self.M = len(self.cols["whp"])

    def predict(self, edit=None) -> np.ndarray:
        cols = self.cols if edit is None else edit.apply(self.cols, GILBERT_INPUTS)
        return np.asarray(self.model.predict(cols), np.float64)


class LearnedScorer(Scorer):
    """The MLP and the LSTM: one pass of scoring.py per ``predict``: fp32 network outputs, the
    pass's own device buffer on the native routes, a numpy array from the oracle. ``what`` names
    the job in the pass's notices. LSTM: an edit acts on the series-sorted row table and a
    prediction belongs to the last row of its window."""

    learned = True

    def __init__(self, pred, table: dict, what: str, piece_rows: int = 0):
        if pred.name == "lstm":
            ps = LstmPass(pred, table, f"LSTM {what} scoring")
        else:
            ps = MlpPass(pred, table, f"MLP {what} scoring", resident=True, piece_rows=piece_rows)
        self.pred, self.ps, self.M, self.rows = pred, ps, ps.M, ps.rows
        self.native, self.on_device = ps.native, ps.on_device
        self.y_scale, self.y_shift = target_scale(pred.pipe)
        if self.on_device:  # the device assembly reads an int32 device vector
            self.perm_device, self.perm_dtype = pred.device, torch.int32

    def predict(self, edit=None):
        return self.ps.score(edit)

    def check_device_errors(self) -> None:
        self.pred.eng.check_device_errors()


def scorer_for(pred, table: dict, what: str, piece_rows: int = 0) -> Scorer:
    scorer = GilbertScorer(pred, table) if pred.name == "gilbert" else LearnedScorer(pred, table, what, piece_rows)
    if scorer.M < 1:
        raise ValueError(f"no row can be scored: every series is shorter than the window of {pred.seq_len} rows")
    return scorer


# ---------------------------------------------------------------------- permutations
class Permutations:
    """The permutations of a run, one per ``draw``: drawn by ``torch.randperm`` from a
    ``torch.Generator`` seeded with ``seed`` on the device that scores, in the order of the draws,
    or injected. ``perms``: None, a tensor of ``shape`` (the last axis: the n rows) or a callable;
    ``axes`` names the tensor's axes and ``call`` the callable's arguments in the refusals."""

    gen = None

    def __init__(self, perms, shape: tuple, axes: str, call: str):
        if isinstance(perms, (torch.Tensor, np.ndarray)):
            perms = torch.as_tensor(perms)
            if tuple(perms.shape) != tuple(shape):
                raise ValueError(f"perms must be {''.join(f'[{d}]' for d in shape)} ({axes}), got {tuple(perms.shape)}")
        elif perms is not None and not callable(perms):
            raise TypeError(f"perms: a tensor {''.join(f'[{a}]' for a in axes.split(', '))} or a callable {call} -> perm")
        self.perms, self.n = perms, shape[-1]

    def bind(self, scorer: Scorer, seed: int) -> None:
        """In front of the pass loop: the generator, or the one conversion / upload of a tensor."""
        self.scorer = scorer
        if self.perms is None:
            self.gen = torch.Generator(device=scorer.perm_device)
            self.gen.manual_seed(seed)
        elif isinstance(self.perms, torch.Tensor):
            self.perms = scorer.own_perms(self.perms)

    def draw(self, index: tuple, args: tuple) -> torch.Tensor:
        """The next permutation: element ``index`` of an injected tensor, or ``perms(*args)``."""
        s, n = self.scorer, self.n
        if self.gen is not None:
            return torch.randperm(n, generator=self.gen, device=s.perm_device, dtype=s.perm_dtype)
        if callable(self.perms):
            perm = s.own_perms(torch.as_tensor(self.perms(*args)))
            if perm.shape != (n,):
                raise ValueError(f"perms({', '.join(map(repr, args))}) gave {tuple(perm.shape)}, not [{n}]")
            return perm
        return self.perms[index]


# ---------------------------------------------------------------------- the tail of a job
def comma_list(text: str | None):
    """``a, b,,c`` -> [a, b, c]; None stays None (the option was not given)."""
    return [v.strip() for v in text.split(",") if v.strip()] if text is not None else None


def other_rank(model: str, out_path: str):
    """One process on one device: rank 0 alone works and writes; another rank's result, else None."""
    if int(os.environ.get("RANK", "0")) != 0:
        return {"model": model, "out": out_path, "skipped": True}
    return None


def write_csv(path: str, header, rows) -> None:
    """``header`` and the ``rows`` (an iterable of cell lists). Atomic (tmp + rename)."""
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    tmp = path + ".tmp"
    with open(tmp, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(header)
        w.writerows(rows)
    os.replace(tmp, path)
