"""One scoring pass over a table: what the prediction job (predict.py) runs once and the
permutation-importance job (importance.py) runs ``1 + columns x repeats`` times (the response and
attribution jobs, response.py and explain.py, run it in the same way).

A pass is built once per table from a :class:`~wellflow.predict.Predictor`. It owns the engine and
its batch, the piece size, the preallocated device buffers and the choice between the three input
routes:

* device assembly (native engine, F <= ``ASSEMBLE_MAX_F``): csrc/features.hip builds the engine's
  input rows from the raw columns; the MLP reads ``[chunk][Fp]`` bf16 slices of a piece in place,
  the LSTM reads its windows in place from the fp32 row table (:meth:`NativeLSTM.forward_windows`);
* host assembly with the native engine (wider tables): ``FeaturePipeline.features`` builds the rows,
  they are uploaded, and the same device loop scores them;
* the fp32 oracle (CPU, or fp32 on a GPU): host rows through the PyTorch engine.

``score(edit)`` returns the network outputs as fp32 ``[M]``: a device tensor (the pass's own
buffer) on the native routes, a numpy array from the oracle. ``edit`` says how the table is edited
for this pass: :class:`PermutedColumn` (one source column read through a permutation,
importance.py), :class:`ConstantColumn` (one source column set to one constant in every row,
response.py), :class:`PermutedSet` (every source column of a set read through one permutation,
explain.py) or :class:`RowValues` (one continuous source column set to its own value in every row,
setpoint.py); without an edit the table is scored as it is. An edit knows two things: how to apply
itself to a host table, and what it tells the device assembly about rows ``[a, b)``.
"""
from __future__ import annotations

import typing

import numpy as np
import torch

from .data.features import SeriesWindows, window_starts

HBM_TABLE_FRACTION = 8  # an assembled MLP table above 1/8 of HBM is assembled and scored piece by piece


def permuted(table: dict, col: str, perm) -> dict:
    t = dict(table)
    t[col] = np.asarray(table[col])[np.asarray(perm, dtype=np.int64)]
    return t


def constant(table: dict, col: str, value) -> dict:
    """The table with column ``col`` set to ``value`` in every row: a label (str) gives an object
    column, anything else a float32 column (the pipeline casts continuous columns to float32)."""
    n = len(next(iter(table.values())))
    t = dict(table)
    t[col] = np.full(n, value, object) if isinstance(value, str) else np.full(n, value, np.float32)
    return t


def _host_perm(perm) -> np.ndarray:
    return torch.as_tensor(perm).cpu().numpy()


class PermutedColumn(typing.NamedTuple):
    """Source column ``k`` (the kernel's source order) read through ``perm``: a vector over ALL rows,
    int32 on the device for the device assembly."""

    k: int
    perm: typing.Any
    what = "a permuted pass"

    def apply(self, table: dict, names) -> dict:
        return permuted(table, names[self.k], _host_perm(self.perm))

    def assemble_args(self, a: int, b: int) -> dict:
        return {"perm": self.perm[a:b], "perm_col": self.k}


class ConstantColumn(typing.NamedTuple):
    """Source column ``k`` set to a constant. ``host``: the label (str) of a categorical column or
    the np.float32 raw value of a continuous one, what the host routes write into the table;
    ``dev``: the same value as a one-element device tensor (the int32 label code / the float32
    value: an element of a grid that was uploaded once), what the device assembly reads."""

    k: int
    host: typing.Any
    dev: typing.Any = None
    what = "a constant pass"

    def apply(self, table: dict, names) -> dict:
        return constant(table, names[self.k], self.host)

    def assemble_args(self, a: int, b: int) -> dict:
        return {"const_col": self.k, "const_value": self.dev}


class PermutedSet(typing.NamedTuple):
    """A SET of source columns read through one permutation ``perm`` (as :class:`PermutedColumn`).
    ``host``: the source-column indices, what the host routes permute one by one; ``dev``: the set's
    bitmask, a row of ``ops.native.column_masks`` on the device (a job uploads the masks of all its
    passes once and a pass points at its row), what the device assembly reads."""

    host: tuple
    dev: typing.Any
    perm: typing.Any
    what = "a pass with a set of permuted columns"

    def apply(self, table: dict, names) -> dict:
        pn = _host_perm(self.perm)
        for s in self.host:
            table = permuted(table, names[s], pn)
        return table

    def assemble_args(self, a: int, b: int) -> dict:
        return {"perm": self.perm[a:b], "col_set": self.dev}


class RowValues(typing.NamedTuple):
    """Continuous source column ``k`` set to its own value in every row (setpoint.py). ``values``:
    one float32 raw value per row of the table, a device vector for the device assembly (a numpy
    array or a tensor for the host routes, which write it into the table as host float32);
    ``ident``: the identity index vector over all rows, int32 on the device and uploaded once by
    the job: rows ``[a, b)`` read ``values`` through ``ident[a:b]``, so a piece gathers from the
    whole vector."""

    k: int
    values: typing.Any
    ident: typing.Any = None
    what = "a pass with per-row values"

    def apply(self, table: dict, names) -> dict:
        t = dict(table)
        t[names[self.k]] = np.ascontiguousarray(torch.as_tensor(self.values).cpu().numpy(), dtype=np.float32)
        return t

    def assemble_args(self, a: int, b: int) -> dict:
        return {"perm": self.ident[a:b], "perm_col": self.k, "perm_values": self.values}


class _Pass:
    """What the MLP and the LSTM pass share. ``table``: the rows in the order they are scored;
    ``M``: predictions per pass; ``rows``: the row of the GIVEN table each prediction belongs to
    (None: every row, in order)."""

    dtype = torch.float32  # of the assembled rows
    res = None  # ResidentColumns: the raw columns on the device, when they are uploaded once

    def __init__(self, pred, table: dict, M: int, what: str):
        pipe = pred.pipe
        self.pred, self.pipe, self.table, self.M = pred, pipe, table, int(M)
        self.names = [ix.column for ix in pipe.indexers] + list(pipe.continuous)  # the kernel's source order
        self.native = self.on_device = False
        if self.M < 1:
            return  # nothing to score: no engine is built
        self.eng = pred._engine(self.M)
        self.B = pred.eng_batch
        self.native = pred.native
        self.on_device = self.native and pred._device_assembly(what)

    def _resident(self, codes, cont):
        from .ops.native import ResidentColumns

        pipe = self.pipe
        return ResidentColumns(codes, cont, *pipe.block_spec(), *pipe.scale(), self.pred.n_features, self.pred.device)

    def _features(self, edit=None) -> np.ndarray:
        """The host pipeline's rows of the table, edited by ``edit``."""
        return self.pipe.features(self.table if edit is None else edit.apply(self.table, self.names))

    def _input_format(self, X: torch.Tensor) -> torch.Tensor:
        return X

    def assemble(self, a: int, b: int, edit=None, host=None) -> torch.Tensor:
        """Rows [a, b) of the table as engine input, in the pass's piece buffer. Device assembly:
        the table as it is or, from resident columns only, edited by ``edit``. ``host``: the
        host-built rows of the whole table instead (host assembly with the native engine)."""
        X = self.X[: b - a]
        if host is not None:
            X.copy_(self._input_format(torch.from_numpy(host[a:b])))
        elif edit is not None:
            if self.res is None:
                raise ValueError(f"{edit.what} reads resident columns (resident=True)")
            self.res.assemble(self.dtype, rows=(a, b), out=X, **edit.assemble_args(a, b))
        elif self.res is not None:
            self.res.assemble(self.dtype, rows=(a, b), out=X)
        else:  # this piece's raw columns alone go up
            self._resident(self.codes[:, a:b], self.cont[:, a:b]).assemble(self.dtype, out=X)
        return X

    def score(self, edit=None):
        """Network outputs fp32 [M] of the table, edited by ``edit`` (None: as it is)."""
        if not self.native:
            return self._score_host(self._features(edit))
        host = None if self.on_device else self._features(edit)
        for a, b in self.pieces:
            self.forward(self.assemble(a, b, edit, host), a)
        return self.p


class MlpPass(_Pass):
    """``resident``: upload the raw columns once (a run of many passes; needed for ``perm``) instead
    of piece by piece (one pass: at most one piece's raw columns and one assembled piece are on the
    device). ``piece_rows``: rows per piece, rounded down to whole engine batches; 0 = what fits
    in 1/``HBM_TABLE_FRACTION`` of HBM."""

    dtype = torch.bfloat16

    def __init__(self, pred, table: dict, what: str = "MLP scoring", resident: bool = False, piece_rows: int = 0):
        n = len(next(iter(table.values())))
        super().__init__(pred, table, n, what)
        self.rows = None
        if not self.native:
            return
        dev, B, Fp = pred.device, self.B, self.eng.Fp
        limit = piece_rows if piece_rows > 0 else \
            torch.cuda.get_device_properties(dev).total_memory // HBM_TABLE_FRACTION // (Fp * 2)
        piece = max(B, limit // B * B)
        self.pieces = [(a, min(n, a + piece)) for a in range(0, n, piece)]
        self.X = torch.empty((min(piece, n), Fp), dtype=torch.bfloat16, device=dev)
        self.p = torch.empty(n, device=dev)
        if self.on_device:
            self.codes, self.cont = self.pipe.raw_columns(table)
            if resident:
                self.res = self._resident(self.codes, self.cont)

    def _input_format(self, X):
        return self.eng.to_input_format(X)

    def forward(self, X: torch.Tensor, a: int = 0) -> None:
        """The assembled piece ``X`` that starts at row ``a`` -> ``p[a : a + len(X)]``."""
        B, m = self.B, X.shape[0]
        for c in range(0, m, B):  # [chunk][Fp] slices read in place; the last one may be short
            self.p[a + c : a + min(c + B, m)].copy_(self.eng.forward(X[c : c + B]))

    def _score_host(self, X: np.ndarray) -> np.ndarray:
        X, B = torch.from_numpy(X), self.B
        p = np.empty(self.M, np.float32)
        for a in range(0, self.M, B):
            p[a : a + B] = self.eng.forward(X[a : a + B]).float().cpu().numpy()
        return p


class LstmPass(_Pass):
    """The rows are grouped into series as training grouped them; a window predicts its last row.
    The row table is one piece: the raw columns go up once and the windows are read in place."""

    def __init__(self, pred, table: dict, what: str = "LSTM scoring"):
        n, T = len(next(iter(table.values()))), pred.seq_len
        stable, ids, order = pred._sorted_series(table, n)
        self.starts = np.asarray(window_starts(n, T, ids), np.int64)
        super().__init__(pred, stable, len(self.starts), what)
        self.T, self.rows, self.pieces = T, order[self.starts + T - 1], [(0, n)]
        if not self.native:
            return
        dev, B, W = pred.device, self.B, self.M
        self.X = torch.empty((n, pred.n_features), dtype=torch.float32, device=dev)
        self.win = SeriesWindows(self.X, torch.from_numpy(self.starts).to(dev), T)
        # window ids per engine launch (whole batches of 64-row tiles), the last chunk padded by repeating a valid id
        self.chunks = [(a, min(B, W - a), torch.arange(a, a + B, device=dev).clamp_(max=min(a + B, W) - 1))
                       for a in range(0, W, B)]
        self.p = torch.empty(W, device=dev)
        if self.on_device:
            self.res = self._resident(*self.pipe.raw_columns(stable))

    def forward(self, X: torch.Tensor = None, a: int = 0) -> None:
        """The windows of the row table (``win`` reads the piece buffer in place) -> ``p``."""
        for a, m, ids in self.chunks:
            self.p[a : a + m].copy_(self.eng.forward_windows(self.win, ids)[:m])  # the padding dropped

    def _score_host(self, X: np.ndarray) -> np.ndarray:
        win, B, W = SeriesWindows(X, self.starts, self.T), self.B, self.M
        p = np.empty(W, np.float32)
        for a in range(0, W, B):
            xb = torch.from_numpy(np.ascontiguousarray(win[np.arange(a, min(a + B, W))]))
            p[a : a + B] = self.eng.forward(xb).float().cpu().numpy()
        return p
