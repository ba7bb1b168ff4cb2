"""The edit values of a scoring pass (wellflow/scoring.py) on the CPU: each kind applied to a host
table against the table edited by hand with ``permuted`` / ``constant``, what it tells the device
assembly about a piece, and ``score(edit)`` of the fp32 oracle passes against scoring the hand-edited
table as it is."""
import numpy as np
import pytest
import torch

from wellflow.data.features import FeaturePipeline
from wellflow.data.io import load_table
from wellflow.data.schema import parse_schema
from wellflow.models import registry
from wellflow.scoring import ConstantColumn, LstmPass, MlpPass, PermutedColumn, PermutedSet, constant, permuted
from wellflow.utils.checkpoint import save_mdl

NAMES = "well,field,t,whp,choke,glr,temp,water_cut,dsp,flow"
TYPES = "string,string,int,float,float,float,float,float,float,float"


def _hand(table, names, edit):
    """The table edited with the module functions alone."""
    if isinstance(edit, PermutedColumn):
        return permuted(table, names[edit.k], np.asarray(edit.perm))
    if isinstance(edit, ConstantColumn):
        return constant(table, names[edit.k], edit.host)
    for s in edit.host:
        table = permuted(table, names[s], np.asarray(edit.perm))
    return table


def _edits(names, n, seed, skip=()):
    """One edit of each kind (a categorical and a continuous constant) over the source columns
    ``names``, none of them touching a column of ``skip``."""
    rng = np.random.default_rng(seed)
    ok = [k for k, c in enumerate(names) if c not in skip]
    perm = torch.from_numpy(rng.permutation(n))
    assert not np.array_equal(perm.numpy(), np.arange(n))
    return {"permuted": PermutedColumn(ok[-1], perm),
            "constant_label": ConstantColumn(ok[0], "f1"),
            "constant_value": ConstantColumn(ok[-2], np.float32(1.25)),
            "set": PermutedSet((ok[0], ok[2], ok[-1]), None, perm)}


# ------------------------------------------------------------------ 1. an edit on a host table
@pytest.mark.parametrize("kind", ["permuted", "constant_label", "constant_value", "set"])
def test_edit_applied_to_a_host_table_equals_the_hand_edit(kind):
    names = ["field", "whp", "choke"]  # one categorical and two continuous source columns
    table = {"field": np.asarray(["f0", "f1", "f0", "f2", "f1"], object),
             "whp": np.asarray([1.0, 2.0, 3.0, 4.0, 5.0], np.float32),
             "choke": np.asarray([10.0, 20.0, 30.0, 40.0, 50.0], np.float32),
             "flow": np.asarray([7.0, 8.0, 9.0, 10.0, 11.0], np.float32)}  # no source column: never touched
    perm = torch.tensor([3, 0, 4, 1, 2])
    edit = {"permuted": PermutedColumn(2, perm), "constant_label": ConstantColumn(0, "f2"),
            "constant_value": ConstantColumn(1, np.float32(2.5)), "set": PermutedSet((0, 2), None, perm)}[kind]
    touched = {"permuted": {"choke"}, "constant_label": {"field"}, "constant_value": {"whp"}, "set": {"field", "choke"}}[kind]
    keep = {c: v.copy() for c, v in table.items()}
    got, want = edit.apply(table, names), _hand(table, names, edit)
    assert list(got) == list(want) == list(table)
    for c in table:
        assert got[c].dtype == want[c].dtype and np.array_equal(got[c], want[c]), c
        if c in touched:
            assert got[c] is not table[c] and not np.array_equal(got[c], table[c]), c
        else:
            assert got[c] is table[c], c  # the same object, not a copy
        assert np.array_equal(table[c], keep[c])  # the given table is left as it was
    if kind == "set":
        assert got["field"].tolist() == ["f2", "f0", "f1", "f1", "f0"] and got["choke"].tolist() == [40, 10, 50, 20, 30]
    if kind == "constant_value":
        assert got["whp"].dtype == np.float32 and got["whp"].tolist() == [2.5] * 5


def test_edit_tells_the_device_assembly_about_a_piece():
    perm = torch.arange(10, dtype=torch.int32).flip(0)
    one, mask = torch.zeros(1), torch.ones(1, dtype=torch.int32)
    args = PermutedColumn(3, perm).assemble_args(2, 7)
    assert sorted(args) == ["perm", "perm_col"] and args["perm_col"] == 3
    assert torch.equal(args["perm"], perm[2:7]) and args["perm"].data_ptr() == perm[2:7].data_ptr()  # a view
    args = ConstantColumn(1, np.float32(0.0), one).assemble_args(2, 7)
    assert sorted(args) == ["const_col", "const_value"] and args["const_col"] == 1 and args["const_value"] is one
    args = PermutedSet((0, 3), mask, perm).assemble_args(2, 7)
    assert sorted(args) == ["col_set", "perm"] and args["col_set"] is mask and torch.equal(args["perm"], perm[2:7])
    with pytest.raises(AttributeError):  # immutable values
        PermutedColumn(3, perm).k = 4


# ------------------------------------------------------------------ 2. score(edit) on the oracle passes
@pytest.fixture(scope="module")
def predictors(tmp_path_factory):
    """The sizes of the jobs' CPU tests: MLPRegressor(18, (256, 256)) on 8 wells x 125 steps and an
    LSTM (T = 8, H = 16) on 3 wells x 40 steps, both as fp32 CPU predictors."""
    from wellflow.models.lstm import LSTMRegressor
    from wellflow.models.mlp import MLPRegressor
    from wellflow.predict import Predictor

    sp = str(tmp_path_factory.mktemp("scoring")) + "/"
    schema = parse_schema(NAMES, TYPES)
    out = {}
    for name, (wells, steps), job in (("mlp", (8, 125), None),
                                      ("lstm", (3, 40), {"seq_len": 8, "group_col": "well", "hidden": 16})):
        table = load_table("synth", schema, synth_wells=wells, synth_steps=steps, seed=3)
        pipe = FeaturePipeline(schema, "flow", standardize_target=True).fit(table)
        torch.manual_seed(0)
        ref = MLPRegressor(pipe.n_features, (256, 256)) if name == "mlp" else LSTMRegressor(pipe.n_features, 16)
        extra = {"features": pipe.state(), **({"job": job} if job else {})}
        save_mdl(sp + f"models/{name}.mdl", name, registry.keras_layers(name, ref), extra)
        out[name] = (Predictor.load(sp + f"models/{name}.mdl", schema, device="cpu", precision="fp32"), table)
    return out


@pytest.mark.parametrize("kind", ["permuted", "constant_label", "constant_value", "set"])
@pytest.mark.parametrize("model", ["mlp", "lstm"])
def test_score_with_an_edit_equals_scoring_the_hand_edited_table(predictors, model, kind):
    pred, table = predictors[model]
    Pass = MlpPass if model == "mlp" else LstmPass
    ps = Pass(pred, table)
    assert not ps.native and ps.names[:2] == ["well", "field"] and len(ps.names) == 9
    n = len(table["flow"])
    # the LSTM's edit acts on the series-sorted row table (ps.table); its series column stays, so
    # that the hand-edited table is grouped into the same series
    edit = _edits(ps.names, n, 5, skip=("well",) if model == "lstm" else ())[kind]
    plain = np.array(ps.score(), copy=True)
    got = np.array(ps.score(edit), copy=True)
    want = Pass(pred, _hand(ps.table, ps.names, edit)).score()
    assert got.dtype == np.float32 and got.shape == (ps.M,) and ps.M == (n if model == "mlp" else 3 * 33)
    assert np.array_equal(got, want)
    assert not np.array_equal(got, plain)  # the edit moved the predictions
    assert np.array_equal(ps.score(), plain)  # and left the pass's table as it was
