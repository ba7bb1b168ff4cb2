"""Sensitivity: how much does the prediction change per unit of an input column, row by row?

    python -m wellflow.sensitivity <model> columnNames columnTypes targetColumn storagePath dataPath
                                   [--columns a,b,..] [--out PATH] [--device D] [--precision P] [--batch-size B] [--header]

The derivative the other what-if jobs can only approximate by differencing two response passes.
Petroleum engineers read a choke model through its elasticities: Gilbert's equation
``q = P S^C / (A R^B)`` has the constant elasticities ``1``, ``C`` and ``-B`` with respect to
``whp``, ``choke`` and ``glr``, and ``gilbert`` is the closed form a learned model's elasticities are
read against. Continuous input columns only (all of them, or ``--columns``).

The rule, per row and picked column ``c``, in float64 on the host after ONE read of the network
outputs ``p`` and the ``[K][n]`` gradients ``g`` (fp32, with respect to the standardised feature):

    v       = (double)p * y_scale + y_shift
    grad_c  = (double)g_c * y_scale / (double)std_c      raw target units per raw column unit
    elast_c = grad_c * (double)x_c / v                   under IEEE rules (x_c: the fp32 raw value)

Routes. ``mlp`` / ``mlp_online`` on a GPU run the fused fp32 gradient kernel (csrc/mlp_f32_grad.hip,
:meth:`NativeMLP.input_gradients_f32`) behind the fp32-native pass of scoring.py, whatever
``--precision`` says: a ``bf16`` request is served in fp32, with one notice, because there is no bf16
gradient kernel. ``--precision fp32``, the CPU, or a shape the kernel refuses (hidden layers other
than (256, 256), more than 512 features) take the oracle route, with one notice: ``torch.autograd``
over the fp32 ``MLPRegressor`` on host-assembled rows. ``gilbert`` runs in host float64 from the
closed form (``dq/dwhp = q/whp``, ``dq/dchoke = C q/choke``, ``dq/dglr = -B q/glr``) with the model's
own constants. ``lstm`` and ``cnn`` are refused.

Output: ``<storagePath>sensitivity/<model>.csv``: the parsed columns, echoed, ``prediction``, then
``grad_<c>`` and ``elast_<c>`` per picked column in source order. Always with a header; floats as
``repr``. Under ``torchrun`` rank 0 alone works and writes.
"""
from __future__ import annotations

import sys

import numpy as np
import torch

from .models.gilbert import GilbertModel
from .predict import Predictor, scoring_job
from .scoring import MlpPass
from .whatif import (GILBERT_INPUTS, comma_list, input_columns, other_rank, select_columns, table_rows, target_scale,
                     write_csv)

NO_COLUMN = "no column to differentiate: the model has no continuous input column"


def _note(s: str) -> None:
    print(s, file=sys.stderr)


def native_precision(name: str, device: str, precision: str) -> str:
    """The precision the job loads the model with: fp32-native for the MLPs on a GPU unless the
    oracle was asked for by name; else what was asked."""
    if device == "auto":
        device = "cuda" if torch.cuda.is_available() else "cpu"
    on_gpu = torch.device(device).type == "cuda"
    return "fp32-native" if name in ("mlp", "mlp_online") and on_gpu and precision != "fp32" else precision


class Sensitivity:
    """``Sensitivity(predictor, piece_rows=0).run(table, columns=None)`` -> ``prediction`` [n],
    ``grad`` and ``elast`` [K][n] (float64), ``columns`` (source order) and ``native``.
    ``piece_rows``: rows of the assembled table per piece on the native path (scoring.py)."""

    def __init__(self, predictor: Predictor, piece_rows: int = 0, note=None):
        if predictor.name == "lstm":
            raise ValueError("sensitivity does not apply to lstm: a gradient through the windows is not built")
        if predictor.name == "cnn":
            raise ValueError("sensitivity does not apply to cnn: the CNN reads only the target's own history, so "
                             "there is no input column to differentiate")
        self.pred, self.piece_rows, self.note = predictor, int(piece_rows), note if note is not None else _note

    def _pick(self, columns) -> list:
        """The picked continuous columns' source indices, in source order."""
        pred, cols = self.pred, input_columns(self.pred)
        if columns is None:
            ks = [k for k, (_, kind) in enumerate(cols) if kind == "continuous"]
        else:
            ks = sorted(select_columns(pred, list(columns), NO_COLUMN, default_all=False,
                                       target="a sensitivity is taken with respect to an INPUT column"))
        for k in ks:
            if cols[k][1] != "continuous":
                raise ValueError(f"column {cols[k][0]!r} is categorical: a derivative needs a continuous column "
                                 f"(sweep its labels with the response job)")
        if not ks:
            raise ValueError(NO_COLUMN)
        return ks

    def run(self, table: dict, columns=None) -> dict:
        pred = self.pred
        ks = self._pick(columns)
        names = [input_columns(pred)[k][0] for k in ks]
        n = table_rows(pred, table)
        x = np.stack([np.asarray(table[c], np.float32).astype(np.float64) for c in names])
        if pred.name == "gilbert":
            v, grad, native = self._gilbert(table, names)
        else:
            p, g, native = self._learned(table, names)
            y_scale, y_shift = target_scale(pred.pipe)
            cont = list(pred.pipe.continuous)
            std = np.asarray([pred.pipe.scale()[1][cont.index(c)] for c in names], np.float64)
            v = p.astype(np.float64) * y_scale + y_shift
            grad = g.astype(np.float64) * y_scale / std[:, None]
        with np.errstate(all="ignore"):
            elast = grad * x / v
        return {"model": pred.name, "native": native, "n": n, "scored": n, "columns": names, "prediction": v,
                "grad": grad, "elast": elast}

    def _gilbert(self, table: dict, names: list):
        model = GilbertModel(correlation=self.pred.extra.get("correlation", "gilbert"))
        _, Bc, Cc, _ = model.constants()
        cols = {k: np.asarray(table[k], np.float64) for k in GILBERT_INPUTS}
        q = np.asarray(model.predict(cols), np.float64)
        expo = {"whp": 1.0, "choke": Cc, "glr": -Bc}
        with np.errstate(all="ignore"):
            grad = np.stack([expo[c] * q / np.asarray(table[c], np.float32).astype(np.float64) for c in names])
        return q, grad, False

    def _learned(self, table: dict, names: list):
        """(p fp32 [n], g fp32 [K][n], native): through the kernel, or torch.autograd on the oracle."""
        pred, pipe = self.pred, self.pred.pipe
        cont = list(pipe.continuous)
        fcol = [pipe.n_features - len(cont) + cont.index(c) for c in names]
        if pred.native and pred.f32:
            ps = MlpPass(pred, table, "MLP sensitivity scoring", piece_rows=self.piece_rows)
            with torch.no_grad():
                G = ps.gradients(fcol)
            pred.eng.check_device_errors()
            return ps.p.cpu().numpy(), G.cpu().numpy(), True  # the one read of the device
        self.note("sensitivity: the fp32 oracle route (torch.autograd over the PyTorch model on host-assembled rows)")
        ref = pred.ref.to(pred.device).float()
        X = torch.from_numpy(pipe.features(table))
        p, g = np.empty(len(X), np.float32), np.empty((len(fcol), len(X)), np.float32)
        for a in range(0, len(X), 65536):
            xb = X[a : a + 65536].to(pred.device).requires_grad_(True)
            out = ref(xb).reshape(-1)
            (gx,) = torch.autograd.grad(out.sum(), xb)
            p[a : a + len(xb)] = out.detach().cpu().numpy()
            g[:, a : a + len(xb)] = gx[:, fcol].t().cpu().numpy()
        return p, g, False


def _write_csv(path: str, table: dict, names: list, result: dict) -> None:
    echo = [np.asarray(table[c]).astype(str) for c in names]
    header = list(names) + ["prediction"] + [f"{s}_{c}" for c in result["columns"] for s in ("grad", "elast")]
    v, grad, elast = result["prediction"], result["grad"], result["elast"]

    def cells(i):
        out = [repr(float(v[i]))]
        for k in range(len(grad)):
            out += [repr(float(grad[k][i])), repr(float(elast[k][i]))]
        return out

    write_csv(path, header, ([e[i] for e in echo] + cells(i) for i in range(result["n"])))


def run_sensitivity(model: str, argv, log=print) -> dict:
    def add_arguments(ap):
        ap.add_argument("--columns", default=None, help="comma-separated continuous input columns (default: all)")

    ns, cfg, schema, out_path, _, load_data = scoring_job(
        "sensitivity", "sensitivity", "sensitivity", "dataPath [--columns a,b,..]", model, argv, add_arguments)
    if skipped := other_rank(model, out_path):
        return skipped
    batch = cfg.batch_size if ns.batch_size is not None else 0
    want = native_precision(model, cfg.device, cfg.precision)
    load = lambda precision: Predictor.load(cfg.mdl_path(model), schema, device=cfg.device, precision=precision,  # noqa: E731
                                            seq_len=cfg.seq_len, group_col=cfg.group_col, batch=batch)
    try:
        pred = load(want)
        if want == "fp32-native" and cfg.precision != want:
            _note(f"sensitivity: --precision {cfg.precision} is served in fp32 (fp32-native): there is no bf16 "
                  f"gradient kernel")
    except ValueError as e:
        if want != "fp32-native" or "fp32-native" not in str(e):
            raise
        _note(f"sensitivity: {e}")  # the kernel refuses the shape: the oracle serves it
        pred = load("fp32")
    job = Sensitivity(pred)
    table = load_data()
    result = job.run(table, comma_list(ns.columns))
    result["out"] = out_path
    _write_csv(out_path, table, schema.names, result)
    log("Rows scored: %d" % result["scored"])
    log("Mean prediction: %f" % float(np.mean(result["prediction"])))
    with np.errstate(all="ignore"):
        order = np.argsort(-np.nanmean(np.abs(result["elast"]), axis=1), kind="stable")
        for k in order:
            g, e = result["grad"][k], result["elast"][k]
            log("%s: mean grad %f, mean |grad| %f, median elast %f" % (result["columns"][k], np.mean(g), np.mean(np.abs(g)),
                                                                     np.nanmedian(e)))
    return result


def main(argv=None) -> int:
    argv = list(sys.argv[1:] if argv is None else argv)
    if not argv or argv[0] in ("-h", "--help"):
        print(__doc__)
        return 0
    run_sensitivity(argv[0], argv[1:])
    return 0


if __name__ == "__main__":
    sys.exit(main())
