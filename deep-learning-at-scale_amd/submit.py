"""``python -m wellflow.submit <model> columnNames columnTypes targetColumn storagePath [dataPath]``

Model names: cnn, mlp, mlp_online, lstm, gilbert (same argv contract as the per-model
scripts under "Artificial intelligence models/" and "Physical model/").

``python -m wellflow.submit predict <model> columnNames columnTypes targetColumn storagePath dataPath``
scores a CSV with the ``.mdl`` a training job saved (wellflow/predict.py).

``python -m wellflow.submit importance <model> columnNames columnTypes targetColumn storagePath dataPath``
ranks the input columns of that ``.mdl`` by permutation importance (wellflow/importance.py).

``python -m wellflow.submit response <model> columnNames columnTypes targetColumn storagePath dataPath --columns a[,b..]``
sweeps one input column at a time over a grid and writes the mean prediction per value, overall and
per ``--by`` group: the model's response curves (wellflow/response.py).

``python -m wellflow.submit explain <model> columnNames columnTypes targetColumn storagePath dataPath``
attributes every row's prediction to the input columns: per-row Shapley contributions in raw target
units that, added to a base value, give the prediction (wellflow/explain.py).

``python -m wellflow.submit setpoint <model> columnNames columnTypes targetColumn storagePath dataPath --column C --want V``
searches, row by row, the value of one continuous input column at which the model predicts the wanted
value (``--want-column COL``: one wanted value per row): the inverse of predict (wellflow/setpoint.py).

``python -m wellflow.submit interval <model> columnNames columnTypes targetColumn storagePath dataPath [--calibrate]``
puts a band around every prediction: ``--calibrate`` scores held-out rows and writes, per ``--by`` group and
level ``--alpha``, the conformal quantile of the residuals; without it the bands are read back and written next
to the predictions as ``lower_<L>`` / ``upper_<L>`` (wellflow/interval.py).
"""
import sys

from .train.job import run_job


def main(argv=None) -> int:
    argv = list(sys.argv[1:] if argv is None else argv)
    if not argv or argv[0] in ("-h", "--help"):
        print(__doc__)
        return 0
    if argv[0] == "predict":  # score a CSV with a saved .mdl (wellflow/predict.py)
        from .predict import main as predict_main

        return predict_main(argv[1:])
    if argv[0] == "importance":  # permutation importance of a saved .mdl's input columns
        from .importance import main as importance_main

        return importance_main(argv[1:])
    if argv[0] == "response":  # response curves of a saved .mdl: one input column set to a grid of values
        from .response import main as response_main

        return response_main(argv[1:])
    if argv[0] == "explain":  # per-row Shapley attribution of a saved .mdl's predictions to its input columns
        from .explain import main as explain_main

        return explain_main(argv[1:])
    if argv[0] == "setpoint":  # per-row bracket search: the value of one input column that gives the wanted prediction
        from .setpoint import main as setpoint_main

        return setpoint_main(argv[1:])
    if argv[0] == "interval":  # conformal prediction bands: calibrate on held-out rows, then apply next to the predictions
        from .interval import main as interval_main

        return interval_main(argv[1:])
    run_job(argv[0], argv[1:])
    return 0


if __name__ == "__main__":
    sys.exit(main())
