"""Integrated gradients: a deterministic per-row attribution of the prediction to the input columns.

    python -m wellflow.explain <model> columnNames columnTypes targetColumn storagePath dataPath
                               --method ig [--steps M=32] [--baseline mean|N] [--columns a,b,..]

The sampling Shapley job (explain.py) needs ``1 + R x K`` scoring passes and its answer moves with
the seed. With the exact input gradient at hand (csrc/mlp_f32_grad.hip) the standard deterministic
attribution is integrated gradients: for a baseline row ``x'`` and feature ``f``

    phi_f = (x_f - x'_f) * mean_j df/dx_f (x' + alpha_j (x - x')),   alpha_j = (2j + 1) / (2M), j < M

(the midpoint rule on the straight path; ``alpha_j`` is the correctly rounded fp32 quotient). The
contributions sum to ``f(x) - f(x')`` up to the quadrature error, which the job reports per row as
``residual``: it is what a user reads to choose ``--steps``. No random draws; one run attributes to
all columns at once.

Baseline. ``mean``: the mean feature row of the scored table, built on the host in float64 from
``pipe.raw_columns`` (a one-hot block holds the label frequencies, with the pipeline's rule for
unknown labels and ``drop_last``; a continuous feature is ``(mean(raw) - mean_c) / std_c``), cast to
fp32. ``N``: the assembled feature row of table row ``N``.

Spans. Every input column is attributed: a categorical column's one-hot block or a continuous
column's one feature, in the assembly kernel's source order. ``--columns`` only selects what is
reported. Per row, in float64 on the host after one read of the device:

    prediction = p * y_scale + y_shift        p: the pass's ordinary score()
    base       = f(x') * y_scale + y_shift    the fp32 forward of the baseline row
    phi_c      = phi[c] * y_scale             phi[c] = sum over the span of (x_f - x'_f) * avg_f (fp64)
    residual   = prediction - base - sum over ALL columns of phi_c

Routes. ``mlp`` / ``mlp_online`` on a GPU: the fused path kernel (csrc/mlp_f32_path.hip: layer 1 and
the last gradient GEMM once per row tile, only the two 256 x 256 products per step) behind the
fp32-native pass, then ``path_attr`` (csrc/score.hip); a ``bf16`` request is served in fp32, with
one notice. ``--precision fp32``, the CPU, hidden shapes other than (256, 256) and more than 512
features take the oracle route, with one notice: ``torch.autograd`` in fp32 over the ``M``
interpolated host-assembled tables, then the same float64 reduction in numpy
(:func:`path_attr_host`). ``gilbert``: the same rule in numpy float64 over raw whp, choke and glr
with the closed-form gradient. ``lstm`` and ``cnn`` are refused.
"""
from __future__ import annotations

import sys

import numpy as np
import torch

from .models.gilbert import GilbertModel
from .scoring import MlpPass
from .whatif import GILBERT_INPUTS, input_columns, select_columns, table_rows, target_scale, write_csv


def _note(s: str) -> None:
    print(s, file=sys.stderr)


def path_alphas(steps: int) -> np.ndarray:
    """The midpoints ``(float)(2j + 1) / (float)(2 steps)`` as fp32: the kernel's own values."""
    return np.arange(1, 2 * steps, 2, dtype=np.float32) / np.float32(2 * steps)


def path_attr_host(X, avg, xb, off, size) -> np.ndarray:
    """``phi[k][i] = sum_{f in span k} ((double)X[i][f] - (double)xb[f]) * (double)avg[i][f]``, the
    sum started at 0.0 and taken in ascending ``f``: the rule of csrc/score.hip ``path_attr``, which
    agrees with this function bit for bit. A span of size 0 gives exactly 0.0."""
    X, avg, xb = (np.asarray(v).astype(np.float64) for v in (X, avg, xb))
    prod = (X - xb[None, : X.shape[1]]) * avg
    phi = np.zeros((len(off), X.shape[0]), np.float64)
    for k, (o, n) in enumerate(zip(off, size)):
        for f in range(int(o), int(o) + int(n)):
            phi[k] = phi[k] + prod[:, f]
    return phi


def refuse_model(name: str) -> None:
    """The models integrated gradients do not serve, with the reason."""
    if name == "lstm":
        raise ValueError("integrated gradients do not apply to lstm: a gradient through the windows is not built")
    if name == "cnn":
        raise ValueError("integrated gradients do not apply to cnn: the CNN reads only the target's own "
                         "history, so there is no input column to attribute a prediction to")


class IntegratedGradients:
    """``IntegratedGradients(predictor, steps=32, baseline="mean", piece_rows=0).run(table,
    columns=None)`` -> ``prediction``, ``base``, ``residual`` [n], ``phi`` [K][n] (float64, the
    reported columns in source order), ``phi_all`` (every input column), ``columns``, ``native``."""

    def __init__(self, predictor, steps: int = 32, baseline="mean", piece_rows: int = 0, note=None):
        refuse_model(predictor.name)
        if not 1 <= int(steps) <= 1024:
            raise ValueError(f"steps must be 1 .. 1024, got {steps}")
        if baseline != "mean":
            try:
                baseline = int(baseline)
            except (TypeError, ValueError):
                raise ValueError(f"baseline must be 'mean' or a row number, got {baseline!r}") from None
        self.pred, self.steps, self.baseline = predictor, int(steps), baseline
        self.piece_rows, self.note = int(piece_rows), note if note is not None else _note

    def _row(self, n: int) -> int:
        if not 0 <= self.baseline < n:
            raise ValueError(f"baseline row {self.baseline} is out of range: the table has rows 0 .. {n - 1}")
        return self.baseline

    def spans(self) -> tuple:
        """(off, size) int32 of every input column's features, in source order."""
        pipe = self.pred.pipe
        off, size = pipe.block_spec()
        nc, F = len(pipe.continuous), pipe.n_features
        return (np.concatenate([off, np.arange(F - nc, F)]).astype(np.int32),
                np.concatenate([size, np.ones(nc)]).astype(np.int32))

    def baseline_row(self, table: dict, n: int) -> np.ndarray:
        """The fp32 baseline feature row ``[n_features]``."""
        pipe = self.pred.pipe
        if self.baseline != "mean":
            i = self._row(n)
            return pipe.features({c: np.asarray(v)[i : i + 1] for c, v in table.items()})[0]
        codes, cont = pipe.raw_columns(table)
        off, size = pipe.block_spec()
        row = np.zeros(pipe.n_features, np.float64)
        for k in range(len(off)):  # one_hot's rule: code j sets feature j of the block where j < size
            row[off[k] : off[k] + size[k]] = np.bincount(codes[k], minlength=size[k])[: size[k]] / float(n)
        mean, std = pipe.scale()
        if len(cont):
            row[pipe.n_features - len(cont):] = (cont.astype(np.float64).mean(axis=1) - mean) / std
        return row.astype(np.float32)

    def run(self, table: dict, columns=None) -> dict:
        pred = self.pred
        have = input_columns(pred)
        picked = sorted(select_columns(pred, columns, "no column to attribute to"))
        n = table_rows(pred, table)
        if pred.name == "gilbert":
            v, base, phi, native = self._gilbert(table, n)
        else:
            y_scale, y_shift = target_scale(pred.pipe)
            p, pb, raw, native = self._learned(table, n)
            v = p.astype(np.float64) * y_scale + y_shift
            base = np.full(n, float(pb) * y_scale + y_shift)
            phi = raw * y_scale
        total = np.zeros(n, np.float64)
        for k in range(len(phi)):
            total = total + phi[k]
        residual = v - base - total
        return {"model": pred.name, "native": native, "n": n, "scored": n, "steps": self.steps,
                "columns": [have[k][0] for k in picked], "prediction": v, "base": base, "phi": phi[picked],
                "phi_all": phi, "residual": residual, "mean_abs": np.abs(phi[picked]).mean(axis=1)}

    def _learned(self, table: dict, n: int):
        """(p fp32 [n], forward of the baseline, phi fp64 [K][n] in network units, native)."""
        pred, m = self.pred, self.steps
        off, size = self.spans()
        xb = self.baseline_row(table, n)
        if pred.native and pred.f32:
            ps = MlpPass(pred, table, "MLP path attribution", piece_rows=self.piece_rows)
            with torch.no_grad():
                xbd = torch.from_numpy(xb).to(ps.p.device)
                phi = ps.path_attributions(xbd, off, size, m)
                pb = pred.eng.forward_f32(xbd[None, :]).clone()
                p = ps.score()
            pred.eng.check_device_errors()
            return p.cpu().numpy(), pb.cpu().numpy()[0], phi.cpu().numpy(), True  # the one read of the device
        self.note("explain: integrated gradients on the fp32 oracle route (torch.autograd over the PyTorch model on "
                  f"{m} interpolated host-assembled tables)")
        ref = pred.ref.to(pred.device).float()
        X = pred.pipe.features(table)
        alphas = path_alphas(m)
        avg, p = np.zeros(X.shape, np.float64), np.empty(n, np.float32)
        xbt = torch.from_numpy(xb).to(pred.device)
        for a in range(0, n, 65536):
            x = torch.from_numpy(X[a : a + 65536]).to(pred.device)
            with torch.no_grad():
                p[a : a + len(x)] = ref(x).reshape(-1).cpu().numpy()
            for al in alphas:  # the interpolated table x' + alpha (x - x') in fp32, the mean in float64
                xi = (xbt + float(al) * (x - xbt)).requires_grad_(True)
                (g,) = torch.autograd.grad(ref(xi).sum(), xi)
                avg[a : a + len(x)] += g.double().cpu().numpy()
        with torch.no_grad():
            pb = float(ref(xbt[None, :]).reshape(-1)[0])
        return p, pb, path_attr_host(X, avg / m, xb, off, size), False

    def _gilbert(self, table: dict, n: int):
        """Gilbert's equation over raw whp, choke and glr in float64: ``dq/dx_c = e_c q / x_c``."""
        model = GilbertModel(correlation=self.pred.extra.get("correlation", "gilbert"))
        _, Bc, Cc, _ = model.constants()
        expo = np.asarray([1.0, Cc, -Bc])
        x = np.stack([np.asarray(table[c], np.float32).astype(np.float64) for c in GILBERT_INPUTS])
        xb = x.mean(axis=1) if self.baseline == "mean" else x[:, self._row(n)]
        q = lambda z: np.asarray(model.predict(dict(zip(GILBERT_INPUTS, z))), np.float64)  # noqa: E731
        d = x - xb[:, None]
        avg = np.zeros_like(x)
        with np.errstate(all="ignore"):
            for al in path_alphas(self.steps).astype(np.float64):
                z = xb[:, None] + al * d
                avg = avg + expo[:, None] * q(z) / z
            phi = d * (avg / self.steps)
        phi[d == 0.0] = 0.0  # a column held at its baseline value contributes nothing, whatever the gradient
        return q(x), np.full(n, float(q(xb[:, None])[0])), phi, False


def write_ig_csv(path: str, table: dict, names: list, result: dict) -> None:
    """The parsed columns, echoed, then prediction, base, phi_<column> per reported column and
    residual. Always with a header; floats as ``repr``; atomic (tmp + rename)."""
    blocks = [result["prediction"], result["base"], *result["phi"], result["residual"]]
    header = list(names) + ["prediction", "base"] + [f"phi_{c}" for c in result["columns"]] + ["residual"]
    echo = [np.asarray(table[c]).astype(str) for c in names]
    write_csv(path, header, ([e[i] for e in echo] + [repr(float(v[i])) for v in blocks] for i in range(result["n"])))
