"""Prediction job: score new well-log rows with a saved ``.mdl``.

    python -m wellflow.predict <model> columnNames columnTypes targetColumn storagePath dataPath
                               [--out PATH] [--seq-len T] [--group-col COL] [--device D] [--precision P] [--header]

A training job (train/job.py) writes the best weights and the fitted feature-pipeline state
into ``<storagePath>models/<model>.mdl``; this job reads that file back, restores the pipeline
(:meth:`FeaturePipeline.from_state`), derives every model shape from the layer shapes, builds
the engine (the native HIP engine on a GPU in bf16, the fp32 PyTorch oracle otherwise) and
writes one prediction per row, in raw target units, next to the echoed input columns.

A scoring job touches every row once, so on the native path the features are assembled ON THE
DEVICE from the raw columns (csrc/features.hip: label codes + continuous values -> the engine's
input rows), not widened on the host and uploaded: one pass of scoring.py, which the
permutation-importance job (importance.py) runs again and again.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

from .config import MODEL_DEFAULTS, RunConfig, build_parser, config_from_namespace
from .data.features import FeaturePipeline, take, window_starts
from .data.io import load_table
from .data.pipeline import _group_ids
from .data.schema import Schema, parse_schema
from .models import registry
from .models.base import note_slow_path
from .models.gilbert import GilbertModel
from .scoring import LstmPass, MlpPass
from .utils import checkpoint as ckpt


def _round_up(x: int, m: int) -> int:
    return (x + m - 1) // m * m


def model_shapes(name: str, layers: list) -> dict:
    """Every model shape, read off the Keras-layout layer shapes of a ``.mdl``."""
    if name in ("mlp", "mlp_online"):
        dense = [p for cls, p in layers if cls == "Dense" and len(p) == 2]
        if len(dense) < 2:
            raise ValueError(f"{name} .mdl holds {len(dense)} Dense layers (needs >= 2)")
        return {"n_features": int(dense[0][0].shape[0]), "mlp_hidden": tuple(int(W.shape[1]) for W, _ in dense[:-1])}
    if name == "lstm":
        p = layers[0][1]
        if len(p) != 12:
            raise ValueError(f"lstm .mdl: first layer holds {len(p)} parameters (needs the 12 of a Keras LSTM)")
        return {"n_features": int(p[0].shape[0]), "hidden": int(p[0].shape[1])}
    if name == "cnn":
        W, Wd = layers[0][1][0], layers[3][1][0]
        filters, in_ch, kernel = int(W.shape[0]), int(W.shape[1]), int(W.shape[2])
        if Wd.shape[0] % filters:
            raise ValueError(f"cnn .mdl: dense input {Wd.shape[0]} is not a multiple of {filters} filters")
        return {"n_features": in_ch, "cnn_filters": filters, "cnn_kernel": kernel,
                "cnn_input_len": int(Wd.shape[0]) // filters + kernel - 1, "cnn_outputs": int(Wd.shape[1])}
    raise ValueError(f"no learned model named {name!r}")


class Predictor:
    """A saved model + its feature pipeline, ready to score tables (dict of columns)."""

    def __init__(self, name: str, schema: Schema, extra: dict, device, native: bool, batch: int = 0):
        self.name, self.schema, self.extra = name, schema, extra
        self.device, self.native, self.batch = device, native, int(batch)
        self.pipe: FeaturePipeline | None = None
        self.ref = None
        self.eng = None
        self.cfg: RunConfig | None = None
        self.seq_len, self.group_col = 0, ""
        self.piece_rows = 0  # rows of the assembled MLP table per piece (0: what fits in 1/8 of HBM; scoring.py)

    # ------------------------------------------------------------------ loading
    @classmethod
    def load(cls, mdl_path: str, schema: Schema, device: str = "auto", precision: str = "bf16", seq_len: int = 64,
             group_col: str = "", batch: int = 0) -> "Predictor":
        """``batch``: rows (windows) per engine launch; 0 = the device-filling batch of the model
        family, capped at the first table's size."""
        if not os.path.exists(mdl_path):
            raise FileNotFoundError(f"no saved model at {mdl_path} (train it first: python -m wellflow.submit <model> ...)")
        name, layers, extra = ckpt.load_mdl(mdl_path)
        if name not in MODEL_DEFAULTS:
            raise ValueError(f"{mdl_path}: unknown model {name!r}")
        if device == "auto":
            device = "cuda" if torch.cuda.is_available() else "cpu"
        dev = torch.device(device)
        if dev.type == "cuda" and dev.index is None:
            # an indexed device: the engines compare tensors' devices with their own (the MLP's
            # in-place input path, the LSTM's window ids), and "cuda" != "cuda:0"
            dev = torch.device("cuda", torch.cuda.current_device())
        self = cls(name, schema, extra, dev, dev.type == "cuda" and precision == "bf16", batch)
        if name == "gilbert":
            return self
        if extra.get("features") is None:
            raise ValueError(f"{mdl_path} holds no feature-pipeline state (extra['features']): it was not written "
                             f"by a training job, so new data cannot be encoded the way the model was trained")
        shp = model_shapes(name, layers)
        job = extra.get("job") or {}
        self.seq_len = int(job.get("seq_len", seq_len))
        self.group_col = str(job.get("group_col", group_col) or group_col)
        cfg = RunConfig(model=name, **MODEL_DEFAULTS[name])
        cfg.seq_len = self.seq_len
        for k, v in shp.items():
            if k != "n_features":
                setattr(cfg, k, v)
        self.cfg, self.n_features = cfg, shp["n_features"]
        # the univariate CNN reads the target's own history: its "feature" is the target series
        self.pipe = FeaturePipeline.from_state(schema, extra["features"],
                                               n_features=None if name == "cnn" else self.n_features)
        self.ref = registry.build_reference(name, cfg, self.n_features, shp.get("cnn_outputs", 1))
        registry.load_keras_layers(name, self.ref, layers)
        self.ref.eval()
        return self

    def _auto_batch(self, n: int) -> int:
        if self.batch > 0:
            b = self.batch
        elif not self.native:
            b = 4096
        elif self.name == "lstm":
            from .models.lstm import NativeLSTM

            b = NativeLSTM.full_grid_batch(self.cfg.hidden, self.device)
        elif self.name == "cnn":
            b = 1024
        else:
            from .models.mlp import NativeMLP

            b = NativeMLP.full_batch(self.device)
        if self.batch <= 0:
            b = min(b, _round_up(max(n, 1), 64))
        if self.native and self.name == "lstm":
            b = max(64, b - b % 64)  # the persistent kernels take whole 64-row tiles
        return max(1, b)

    def _engine(self, n: int):
        """The engine, built on first use through models/registry.py with the saved weights."""
        if self.eng is None:
            b = self._auto_batch(n)
            eng, ref = registry.build_engine(self.name, self.cfg, self.n_features, getattr(self.cfg, "cnn_outputs", 1),
                                             b, self.device, self.native)
            registry.reference_to_engine(self.ref, eng)
            self.eng, self.eng_batch = eng, b
        return self.eng

    # ------------------------------------------------------------------ scoring
    def predict_table(self, table: dict):
        """Predictions in raw target units, aligned with the table's rows in their given order
        (NaN where a row has no prediction: no window ends there). ``cnn``:
        ``(window_end_row [W], forecasts [W][O])``."""
        n = len(next(iter(table.values()))) if table else 0
        if self.name == "gilbert":
            need = [k for k in ("whp", "choke", "glr") if k not in table]
            if need:
                raise ValueError(f"gilbert needs the columns whp, choke, glr; the data lacks {need}")
            model = GilbertModel(correlation=self.extra.get("correlation", "gilbert"))
            return model.predict({k: np.asarray(table[k], np.float64) for k in ("whp", "choke", "glr")})
        if self.name == "cnn":
            return self._predict_cnn(table, n)
        out = np.full(n, np.nan, np.float32)
        if n == 0:
            return out
        ps = LstmPass(self, table) if self.name == "lstm" else MlpPass(self, table, piece_rows=self.piece_rows)
        if ps.M:
            with torch.no_grad():
                p = ps.score()
            p = np.asarray(self.pipe.inverse_target(torch.as_tensor(p).cpu().numpy()), np.float32)
            self.eng.check_device_errors()
            if ps.rows is None:
                return p
            out[ps.rows] = p
        return out

    def _device_assembly(self, what: str) -> bool:
        from .ops.native import ASSEMBLE_MAX_F

        if self.n_features <= ASSEMBLE_MAX_F:
            return True
        note_slow_path(what, "features are assembled on the host",
                       f"{self.n_features} features > {ASSEMBLE_MAX_F} (the device assembly's LDS tile)",
                       f"F={self.n_features}")
        return False

    def _sorted_series(self, table: dict, n: int):
        """Rows grouped into series as training grouped them (stable sort: file order is time
        order inside a series): (sorted table, series id per sorted row, order)."""
        ids, _ = _group_ids(table, self.schema, self.group_col if self.group_col in table else "")
        if ids is None:
            return table, None, np.arange(n)
        order = np.argsort(ids, kind="stable")
        return take(table, order), ids[order], order

    def _predict_cnn(self, table: dict, n: int):
        L, O = self.cfg.cnn_input_len, self.cfg.cnn_outputs
        if self.pipe.target not in table:
            raise ValueError(f"cnn forecasts the target's own history: the data lacks the column {self.pipe.target!r}")
        stable, ids, order = self._sorted_series(table, n)
        y = self.pipe.target_values(stable)  # standardised, as in training
        # every length-L window inside a series, those whose horizon lies past the data included
        starts = np.asarray(window_starts(n, L, ids), np.int64)
        W = len(starts)
        end_rows = order[starts + L - 1] if W else np.zeros(0, np.int64)
        fc = np.zeros((W, O), np.float32)
        if W:
            eng = self._engine(W)
            B = self.eng_batch
            X = y[starts[:, None] + np.arange(L)[None, :]].astype(np.float32)[:, :, None]
            with torch.no_grad():
                for a in range(0, W, B):
                    p = eng.forward(torch.from_numpy(X[a : a + B]).to(self.device))
                    fc[a : a + B] = p.float().reshape(-1, O).cpu().numpy()
            eng.check_device_errors()
            fc = np.asarray(self.pipe.inverse_target(fc), np.float32)
        return end_rows, fc


# ---------------------------------------------------------------------- the job
def _numeric_target(table: dict, target: str):
    """The raw target column as float64, or None when it is missing or does not parse."""
    if target not in table:
        return None
    try:
        return np.asarray([float(v) for v in table[target]], np.float64) if np.asarray(
            table[target]).dtype == object else np.asarray(table[target], np.float64)
    except (TypeError, ValueError):
        return None


def _cnn_mse(pred: "Predictor", table: dict, end_rows, fc):
    """MSE of the forecasts whose horizon rows exist (same series, raw units); None without any."""
    y = _numeric_target(table, pred.pipe.target)
    if y is None or not len(end_rows):
        return None, 0
    n = len(y)
    _, ids, order = pred._sorted_series(table, n)
    pos = np.empty(n, np.int64)
    pos[order] = np.arange(n)  # row -> position in the series-sorted table
    ys = y[order]
    sid = np.zeros(n, np.int64) if ids is None else ids
    O = fc.shape[1]
    p = pos[end_rows][:, None] + 1 + np.arange(O)[None, :]
    ok = p < n
    pc = np.minimum(p, n - 1)
    ok &= sid[pc] == sid[pos[end_rows]][:, None]
    if not ok.any():
        return None, 0
    d = fc.astype(np.float64)[ok] - ys[pc][ok]
    return float(np.mean(d * d)), int(ok.sum())


def _write_csv(path: str, table: dict, names: list, pred_cols: dict, header: bool) -> None:
    """The parsed table's columns + the prediction column(s); NaN -> empty cell. Atomic."""
    import pyarrow as pa
    import pyarrow.csv as pacsv

    cols = {}
    for c in names:
        v = np.asarray(table[c])
        cols[c] = pa.array(list(v)) if v.dtype == object else pa.array(v)
    for c, v in pred_cols.items():
        v = np.asarray(v)
        cols[c] = pa.array(v, mask=np.isnan(v))
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    tmp = path + ".tmp"
    pacsv.write_csv(pa.table(cols), tmp, write_options=pacsv.WriteOptions(include_header=header))
    os.replace(tmp, path)


def scoring_job(module: str, noun: str, kind: str, usage: str, model: str, argv, add_arguments=None):
    """The front matter of a job that scores a saved model (``python -m wellflow.<module>``): the
    parser (+ the job's own arguments, + ``--out``), the run configuration and the schema.
    Returns ``(ns, cfg, schema, out_path, load_predictor, load_data)``; ``out_path``, the ``noun``
    CSV, defaults to ``<storagePath><kind>/<model>.csv``."""
    ap = build_parser(model)
    ap.prog = f"python -m wellflow.{module} {model}"
    ap.description = f"Usage: python -m wellflow.{module} <model> columnNames columnTypes targetColumn storagePath {usage}"
    if add_arguments is not None:
        add_arguments(ap)
    ap.add_argument("--out", default=None, help=f"{noun} CSV (default <storagePath>{kind}/<model>.csv)")
    ns = ap.parse_args(list(argv))
    cfg = config_from_namespace(model, ns)
    schema = parse_schema(cfg.column_names, cfg.column_types)
    sp = cfg.storage_path
    if sp and not sp.endswith(("/", os.sep)):
        sp += os.sep
    out_path = ns.out or os.path.join(sp + kind, f"{model}.csv")

    def load_predictor() -> Predictor:
        return Predictor.load(cfg.mdl_path(model), schema, device=cfg.device, precision=cfg.precision,
                              seq_len=cfg.seq_len, group_col=cfg.group_col,
                              batch=cfg.batch_size if ns.batch_size is not None else 0)

    def load_data() -> dict:
        return load_table(cfg.data, schema, header=cfg.header, synth_wells=cfg.synth_wells,
                          synth_steps=cfg.synth_steps, seed=cfg.seed)

    return ns, cfg, schema, out_path, load_predictor, load_data


def run_predict(model: str, argv, log=print) -> dict:
    _, cfg, schema, out_path, load_predictor, load_data = scoring_job(
        "predict", "prediction", "predictions", "dataPath", model, argv)
    pred = load_predictor()
    table = load_data()
    n = len(table[schema.names[0]])
    dropped = 0
    if cfg.data not in ("synth", "synthetic", ""):
        from .data import native

        if native.wanted():
            dropped = int(native.read_csv.last_dropped)
    result = {"model": model, "native": pred.native, "rows": n, "dropped": dropped, "mse": None}
    if model == "cnn":
        end_rows, fc = pred.predict_table(table)
        O = fc.shape[1] if fc.ndim == 2 else cfg.cnn_outputs
        full = np.full((n, O), np.nan, np.float32)
        full[end_rows] = fc
        pred_cols = {f"prediction_{k + 1}": full[:, k] for k in range(O)}
        scored = len(end_rows)
        result["mse"], _ = _cnn_mse(pred, table, end_rows, fc)
        result["predictions"] = (end_rows, fc)
    else:
        p = np.asarray(pred.predict_table(table))
        pred_cols = {"prediction": p}
        ok = ~np.isnan(p)
        scored = int(ok.sum())
        y = _numeric_target(table, cfg.target)
        if y is not None and scored:
            d = p[ok].astype(np.float64) - y[ok]
            result["mse"] = float(np.mean(d * d))
        result["predictions"] = p
    result.update(scored=scored, unscored=n - scored)
    result["out"] = out_path
    if int(os.environ.get("RANK", "0")) == 0:
        _write_csv(out_path, table, schema.names, pred_cols, cfg.header)
        log("Rows scored: %d" % scored)
        log("Rows without prediction: %d" % (n - scored))
        if dropped:
            log("Rows dropped by the reader: %d" % dropped)
        if result["mse"] is not None:
            log("Scoring MSE: %f" % result["mse"])
    return result


def main(argv=None) -> int:
    argv = list(sys.argv[1:] if argv is None else argv)
    if not argv or argv[0] in ("-h", "--help"):
        print(__doc__)
        return 0
    run_predict(argv[0], argv[1:])
    return 0


if __name__ == "__main__":
    sys.exit(main())
