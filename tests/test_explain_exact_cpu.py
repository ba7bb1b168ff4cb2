"""Exact Shapley attribution on the CPU (wellflow/shapley_exact.py): the weights against fractions, the rule
against the average over all K! orders, Gilbert against the subset-weight formula, and the CLI's refusals."""
from fractions import Fraction
from itertools import permutations
from math import factorial

import numpy as np
import pytest
import torch

from test_explain_ig_cpu import NAMES, TYPES, _saved
from wellflow.data.io import write_csv
from wellflow.explain import run_explain
from wellflow.predict import Predictor
from wellflow.shapley_exact import ExactShapley, exact_shapley_host, shapley_weights


@pytest.mark.parametrize("K", (1, 2, 9, 12))
def test_weights_against_fractions(K):
    w = shapley_weights(K)
    assert w.shape == (2, K + 1) and w.dtype == np.float64 and w[0, 0] == 0.0 and w[1, K] == 0.0
    for s in range(K + 1):
        if s >= 1:
            assert w[0, s] == float(Fraction(factorial(s - 1) * factorial(K - s), factorial(K)))
        if s < K:
            assert w[1, s] == float(Fraction(factorial(s) * factorial(K - s - 1), factorial(K)))


@pytest.mark.parametrize("K", (1, 3, 4))
def test_rule_against_all_orders(K):
    """phi_c is the mean over all K! orders of the step p(before + c) - p(before). Both sides are float64 sums
    of at most 2^K (K! 2) terms of size max |p|, so they agree to (2^K + 2 K!) 2^-53 max |p|."""
    g = torch.Generator().manual_seed(K)
    net = torch.nn.Sequential(torch.nn.Linear(K + 2, 16), torch.nn.ReLU(), torch.nn.Linear(16, 1))
    x, xb = torch.randn(7, K + 2, generator=g), torch.randn(K + 2, generator=g)
    rows = []
    for i in range(1 << K):  # features 1 .. K are the players; 0 and K + 1 keep the row's own value
        own = torch.tensor([True] + [bool((i >> c) & 1) for c in range(K)] + [True])
        with torch.no_grad():
            rows.append(net(torch.where(own, x, xb)).reshape(-1).numpy())
    p_all = np.stack(rows)
    want = np.zeros((K, 7))
    for order in permutations(range(K)):
        i = 0
        for c in order:
            want[c] += p_all[i | (1 << c)].astype(np.float64) - p_all[i].astype(np.float64)
            i |= 1 << c
    want /= factorial(K)
    got = exact_shapley_host(p_all, K)
    assert np.abs(got - want).max() <= ((1 << K) + 2 * factorial(K)) * 2.0 ** -53 * np.abs(p_all).max()
    assert np.abs(got.sum(0) - (p_all[-1].astype(np.float64) - p_all[0])).max() <= (K << K) * 2.0 ** -53 * np.abs(p_all).max()


def test_gilbert_against_the_subset_weights(tmp_path):
    schema, table, *_, p = _saved(tmp_path, "gilbert")
    pred = Predictor.load(p, schema, device="cpu")
    out = ExactShapley(pred, baseline=2).run(table)
    assert out["columns"] == ["whp", "choke", "glr"] and not out["native"]
    from wellflow.models.gilbert import GilbertModel
    model = GilbertModel(correlation="ros")
    x = np.stack([np.asarray(table[c], np.float32).astype(np.float64) for c in out["columns"]])
    v = {}
    for S in range(8):
        z = np.where(np.asarray([(S >> c) & 1 for c in range(3)], bool)[:, None], x, x[:, 2:3])
        v[S] = np.asarray(model.predict(dict(zip(out["columns"], z))), np.float64)
    for c in range(3):  # sum over S without c of |S|! (2 - |S|)! / 3! (v(S + c) - v(S))
        want = sum(Fraction(factorial(bin(S).count("1")) * factorial(2 - bin(S).count("1")), 6) * (v[S | 1 << c] - v[S])
                   for S in range(8) if not (S >> c) & 1)
        assert np.abs(out["phi"][c] - want).max() <= 16 * 2.0 ** -53 * np.abs(v[7]).max()
    assert np.array_equal(out["prediction"], v[7]) and np.array_equal(out["base"], v[0])
    assert np.abs(out["residual"]).max() <= 32 * 2.0 ** -53 * np.abs(v[7]).max()
    # the baseline row itself: every coalition has one value, so column 0's terms cancel pair by pair, exactly
    assert out["phi"][0, 2] == 0.0 and np.abs(out["phi"][:, 2]).max() <= 16 * 2.0 ** -53 * abs(v[7][2])
    two = ExactShapley(pred, baseline=2).run(table, ["glr", "whp"])  # choke keeps its own value
    assert two["columns"] == ["whp", "glr"] and np.abs(two["base"] - v[2]).max() == 0.0


def test_oracle_route_and_the_job(tmp_path):
    schema, table, pipe, ref, p = _saved(tmp_path)
    path = str(tmp_path / "data.csv")
    write_csv(table, path, columns=NAMES.split(","))
    notes = []
    job = ExactShapley(Predictor.load(p, schema, device="cpu", precision="fp32"), baseline=5, note=notes.append)
    out = job.run(table, ["whp", "well", "glr"])
    assert out["columns"] == ["well", "whp", "glr"] and len(notes) == 1 and "oracle" in notes[0]
    assert np.abs(out["residual"]).max() <= 1e-12 * np.abs(out["prediction"]).max() and out["phi"][0, 5] == 0.0
    with torch.no_grad():
        full = ref(torch.from_numpy(pipe.features(table))).reshape(-1).double().numpy() * pipe.y_std + pipe.y_mean
    assert np.array_equal(out["prediction"], full)
    res = run_explain("mlp", [NAMES, TYPES, "flow", str(tmp_path) + "/", path, "--method", "exact", "--device", "cpu",
                              "--columns", "whp,glr"], log=lambda *a, **k: None)
    assert res["columns"] == ["whp", "glr"] and res["out"].endswith("explain/mlp.csv")
    with open(res["out"]) as f:
        assert f.readline().strip().split(",")[-5:] == ["prediction", "base", "phi_whp", "phi_glr", "residual"]


@pytest.mark.parametrize("model,extra,msg", [
    ("lstm", ["--method", "exact"], "exact Shapley values do not apply to lstm"),
    ("cnn", ["--method", "exact"], "exact Shapley values do not apply to cnn"),
    ("mlp", ["--method", "exact", "--repeats", "4"], "--repeats does not apply to --method exact"),
    ("mlp", ["--method", "exact", "--std"], "--std does not apply to --method exact"),
    ("mlp", ["--method", "exact", "--seed=3"], "--seed does not apply to --method exact"),
    ("mlp", ["--method", "exact", "--steps", "8"], "--steps does not apply to --method exact"),
    ("mlp", ["--method", "exact", "--baseline", "102", "--device", "cpu"], "baseline row 102 is out of range"),
    ("mlp", ["--method", "exact", "--columns", "flow", "--device", "cpu"], "flow"),
    ("mlp", ["--method", "ig", "--repeats", "4"], "--repeats does not apply to --method ig"),  # unchanged
    ("mlp", ["--steps", "8"], "--steps does not apply to --method shapley"),
    ("mlp", ["--baseline", "mean"], "--baseline does not apply to --method shapley"),
])
def test_cli_refusals(tmp_path, model, extra, msg):
    schema, table, *_ = _saved(tmp_path)
    path = str(tmp_path / "data.csv")
    write_csv(table, path, columns=NAMES.split(","))
    with pytest.raises(ValueError, match=msg):
        run_explain(model, [NAMES, TYPES, "flow", str(tmp_path) + "/", path, *extra], log=lambda *a, **k: None)


def test_more_than_twelve_players_are_refused(tmp_path, monkeypatch):
    schema, table, *_, p = _saved(tmp_path)
    job = ExactShapley(Predictor.load(p, schema, device="cpu", precision="fp32"))
    monkeypatch.setattr("wellflow.shapley_exact.select_columns", lambda *a, **k: list(range(13)))
    with pytest.raises(ValueError, match="13 columns > 12; pick the players with --columns"):
        job.run(table)
