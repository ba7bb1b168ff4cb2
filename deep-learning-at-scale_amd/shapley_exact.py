"""Exact Shapley attribution: the quantity the sampling job (explain.py) estimates, by enumeration.

    python -m wellflow.explain <model> columnNames columnTypes targetColumn storagePath dataPath
                               --method exact [--baseline mean|N] [--columns a,b,..]

The game. ``K`` picked input columns (1 .. 12, kept in the assembly kernel's source order) are the
players; for a baseline feature row ``x'`` the value of a coalition ``S`` is the network output
``p(S) = f(the row's own values on the columns of S, x' on the other picked columns)``. Columns
that were not picked keep the row's own values in every coalition. Coalition ``i = 0 .. 2^K - 1``
holds column ``c`` iff bit ``c`` of ``i`` is set.

The rule (:func:`exact_shapley_host`; csrc/mlp_f32_shap.hip agrees with it bit for bit given the
same ``p``). With ``w_in[s] = (s-1)!(K-s)!/K!`` and ``w_out[s] = s!(K-s-1)!/K!``
(:func:`shapley_weights`, rounded once from exact fractions), per row, in float64, in ascending
``i``, one multiply and one add, never contracted:

    phi_c = phi_c + (double)p(S_i) * (w_in[|S_i|] if c in S_i else -w_out[|S_i|])

Per row, in float64 on the host after one read of the device:

    prediction = p(all own) * y_scale + y_shift
    base       = p(none own) * y_scale + y_shift      per row: unpicked columns are the row's own
    phi_c      = phi[c] * y_scale
    residual   = prediction - base - sum over the picked columns of phi_c

The weights of a coalition sum to 0 (1 for all own, -1 for none own), so the residual is float64
rounding only: that is what local accuracy means here. No random draws and no quadrature.

Baseline: ``mean`` or a row number, as integrated gradients build it (integrated.py).

Routes. ``mlp`` / ``mlp_online`` on a GPU: the fused coalition kernel (layer 1 ``K + 1`` times per
row tile, then per coalition a few adds, the 256 x 256 layer and the head, the rule applied where
the output is produced: ``K + 2`` numbers per row leave the kernel) behind the fp32-native pass; a
``bf16`` request is served in fp32, with one notice. ``--precision fp32``, the CPU, hidden shapes
other than (256, 256) and more than 512 features take the oracle route, with one notice: the
``2^K`` host tables ``where(span in S, x, x')`` through the ``torch`` fp32 forward, then
:func:`exact_shapley_host`. ``gilbert``: the same rule in numpy float64 over raw whp, choke and glr.
``lstm`` and ``cnn`` are refused.
"""
from __future__ import annotations

from fractions import Fraction
from math import factorial

import numpy as np
import torch

from .integrated import IntegratedGradients, _note
from .models.gilbert import GilbertModel
from .scoring import MlpPass
from .whatif import GILBERT_INPUTS, input_columns, select_columns, table_rows, target_scale

MAX_COLUMNS = 12  # kMlpShapMaxCols (csrc/kernels.h): 4096 coalitions per row


def shapley_weights(K: int) -> np.ndarray:
    """float64 ``[2][K + 1]``: ``w_in[s]`` (s >= 1) and ``w_out[s]`` (s <= K - 1), each the exact
    fraction rounded once; the unused entries ``w_in[0]`` and ``w_out[K]`` are 0."""
    if not 1 <= int(K) <= MAX_COLUMNS:
        raise ValueError(f"exact Shapley values need 1 .. {MAX_COLUMNS} columns, got {K}")
    K = int(K)
    w = np.zeros((2, K + 1), np.float64)
    for s in range(K + 1):
        if s >= 1:
            w[0, s] = float(Fraction(factorial(s - 1) * factorial(K - s), factorial(K)))
        if s <= K - 1:
            w[1, s] = float(Fraction(factorial(s) * factorial(K - s - 1), factorial(K)))
    return w


def exact_shapley_host(p_all, K: int) -> np.ndarray:
    """``phi [K][n]`` float64 from ``p_all [2^K][n]`` (fp32 network outputs; float64 is taken as
    it is): the module's rule, coalitions in ascending ``i``, a product then a sum per step."""
    p_all = np.asarray(p_all)
    if p_all.ndim != 2 or p_all.shape[0] != 1 << K:
        raise ValueError(f"p_all must be [{1 << K}][n] for {K} columns, got {p_all.shape}")
    w_in, w_out = shapley_weights(K)
    phi = np.zeros((K, p_all.shape[1]), np.float64)
    for i in range(1 << K):
        t, s = p_all[i].astype(np.float64), bin(i).count("1")
        for c in range(K):
            phi[c] = phi[c] + t * (w_in[s] if (i >> c) & 1 else -w_out[s])
    return phi


def refuse_model(name: str) -> None:
    """The models the exact attribution does not serve, with the reason."""
    if name == "lstm":
        raise ValueError("exact Shapley values do not apply to lstm: a window's coalitions against one baseline row "
                         "are not built")
    if name == "cnn":
        raise ValueError("exact Shapley values do not apply to cnn: the CNN reads only the target's own "
                         "history, so there is no input column to attribute a prediction to")


class ExactShapley:
    """``ExactShapley(predictor, baseline="mean", piece_rows=0).run(table, columns=None)`` ->
    ``prediction``, ``base``, ``residual`` [n], ``phi`` [K][n] (float64, the picked columns in
    source order), ``columns``, ``native``, ``scored``, ``mean_abs``."""

    def __init__(self, predictor, baseline="mean", piece_rows: int = 0, note=None):
        refuse_model(predictor.name)
        self.ig = IntegratedGradients(predictor, 1, baseline, piece_rows, note)  # the baseline row and the spans
        self.pred, self.piece_rows, self.note = predictor, int(piece_rows), note if note is not None else _note

    def run(self, table: dict, columns=None) -> dict:
        pred = self.pred
        have = input_columns(pred)
        picked = sorted(select_columns(pred, columns, "no column to attribute to"))
        if len(picked) > MAX_COLUMNS:
            raise ValueError(f"exact Shapley values enumerate 2^K coalitions: {len(picked)} columns > {MAX_COLUMNS}; "
                             "pick the players with --columns (the others keep their own values)")
        n = table_rows(pred, table)
        if pred.name == "gilbert":
            v, base, phi, native = self._gilbert(table, n, picked)
        else:
            y_scale, y_shift = target_scale(pred.pipe)
            pf, p0, raw, native = self._learned(table, n, picked)
            v = pf.astype(np.float64) * y_scale + y_shift
            base = p0.astype(np.float64) * y_scale + y_shift
            phi = raw * y_scale
        total = np.zeros(n, np.float64)
        for k in range(len(phi)):
            total = total + phi[k]
        return {"model": pred.name, "native": native, "n": n, "scored": n, "columns": [have[k][0] for k in picked],
                "prediction": v, "base": base, "phi": phi, "residual": v - base - total,
                "mean_abs": np.abs(phi).mean(axis=1)}

    def _learned(self, table: dict, n: int, picked: list):
        """(pfull fp32 [n], p0 fp32 [n], phi fp64 [K][n] in network units, native)."""
        pred, K = self.pred, len(picked)
        off, size = (v[picked] for v in self.ig.spans())
        xb = self.ig.baseline_row(table, n)
        if pred.native and pred.f32:
            ps = MlpPass(pred, table, "MLP exact attribution", piece_rows=self.piece_rows)
            with torch.no_grad():
                phi, p0 = ps.exact_attributions(torch.from_numpy(xb).to(ps.p.device), off, size)
            pred.eng.check_device_errors()
            return ps.p.cpu().numpy(), p0.cpu().numpy(), phi.cpu().numpy(), True  # the one read of the device
        self.note(f"explain: exact Shapley values on the fp32 oracle route (the PyTorch model on {1 << K} composed "
                  "host-assembled tables)")
        ref = pred.ref.to(pred.device).float()
        X = pred.pipe.features(table)
        member = np.zeros((K, X.shape[1]), bool)  # member[c][f]: feature f belongs to picked column c
        for c in range(K):
            member[c, off[c] : off[c] + size[c]] = True
        p_all = np.empty((1 << K, n), np.float32)
        with torch.no_grad():
            for i in range(1 << K):
                back = np.zeros(X.shape[1], bool)  # the features that take the baseline's value
                for c in range(K):
                    if not (i >> c) & 1:
                        back |= member[c]
                Xi = np.where(back[None, :], xb[None, :], X)
                for a in range(0, n, 65536):
                    x = torch.from_numpy(Xi[a : a + 65536]).to(pred.device)
                    p_all[i, a : a + len(x)] = ref(x).reshape(-1).cpu().numpy()
        return p_all[-1], p_all[0], exact_shapley_host(p_all, K), False

    def _gilbert(self, table: dict, n: int, picked: list):
        """Gilbert's equation over raw whp, choke and glr in float64; the baseline is the columns'
        mean or row N."""
        model = GilbertModel(correlation=self.pred.extra.get("correlation", "gilbert"))
        x = np.stack([np.asarray(table[c], np.float32).astype(np.float64) for c in GILBERT_INPUTS])
        xb = x.mean(axis=1) if self.ig.baseline == "mean" else x[:, self.ig._row(n)]
        q = lambda z: np.asarray(model.predict(dict(zip(GILBERT_INPUTS, z))), np.float64)  # noqa: E731
        K = len(picked)
        p_all = np.empty((1 << K, n), np.float64)
        for i in range(1 << K):
            z = x.copy()
            for c, k in enumerate(picked):
                if not (i >> c) & 1:
                    z[k] = xb[k]
            p_all[i] = q(z)
        return p_all[-1], p_all[0], exact_shapley_host(p_all, K), False
