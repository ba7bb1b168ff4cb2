"""The declared device-state classes (wellflow/train/state_ref.py) and the bit-pattern comparison
the GPU resume tests rest on (tests/test_resume_gpu.py), without a GPU: the engines are built on
the CPU over a stand-in for the kernel library, which is enough to see every buffer they allocate."""
import types

import pytest
import torch

from wellflow.train import state_ref
from wellflow.train.state_ref import compare_states, device_state, images, unclassified


class _NoKernels:
    """Stand-in for wellflow._C: every kernel is a no-op; the two size queries answer."""

    def __getattr__(self, name):
        if name == "cnn_fused_ok":
            return lambda dims, p: True
        if name == "cnn_part_sizes":
            return lambda batch, dims: (8, 8, 8)
        if name.endswith("_scratch_floats"):
            return lambda: 16
        return lambda *a, **k: None


@pytest.fixture
def no_kernels(monkeypatch):
    from wellflow.ops import native

    monkeypatch.setattr(native, "lib", lambda: _NoKernels())
    monkeypatch.setattr(torch.cuda, "get_device_properties",
                        lambda dev: types.SimpleNamespace(multi_processor_count=256))
    for k in ("WELLFLOW_MLP_SPREAD", "WELLFLOW_MLP_STEP128", "WELLFLOW_DW_SLAB", "WELLFLOW_CNN_FUSED"):
        monkeypatch.delenv(k, raising=False)


def _engines():
    from wellflow.models.cnn import CnnLayout, NativeCNN
    from wellflow.models.lstm import NativeLSTM
    from wellflow.models.mlp import NativeMLP

    return {"mlp": NativeMLP(16, (256, 256), 64, device="cpu"),
            "lstm": NativeLSTM(16, 128, 4, 16, device="cpu"),
            "cnn": NativeCNN(CnnLayout(), 8, device="cpu"),
            "cnn_gemm": NativeCNN(CnnLayout(), 8, device="cpu", fused=False)}


def _with_device_buffers(opt):
    # on a GPU the optimizers also hold these (optim/flat.py: allocated when params.is_cuda)
    opt.step_dev = torch.zeros(4)
    opt.clip_state, opt.clip_scratch = torch.zeros(8), torch.zeros(256)
    return opt


def test_every_tensor_attribute_has_exactly_one_class(no_kernels):
    from wellflow.optim.flat import FlatAdam, FlatSGD

    seen = set()
    for name, eng in _engines().items():
        eng.small is None or eng.small.buffers(lambda: 16, "cpu")  # the first launch allocates them
        kw = eng.fused_update_kwargs("adam") if name == "mlp" else {}
        for opt in (FlatAdam(eng.params, eng.grads, **kw), FlatSGD(eng.params, eng.grads)):
            assert unclassified(eng, _with_device_buffers(opt)) == [], name
            seen |= {(type(o).__name__, k) for o in (eng, eng.small, opt) if o is not None
                     for k in state_ref.tensor_attributes(o)}
    # ... and the declaration names nothing that no object has (a renamed buffer leaves no stale row)
    declared = {(c, k) for c, attrs in state_ref.STATE_CLASSES.items() for k in attrs}
    assert declared == seen, (sorted(declared - seen), sorted(seen - declared))
    for attrs in state_ref.STATE_CLASSES.values():
        assert set(attrs.values()) <= {state_ref.CARRIED, state_ref.REBUILT, state_ref.SCRATCH, state_ref.FIXED}


def test_a_buffer_added_later_is_reported(no_kernels):
    from wellflow.optim.flat import FlatSGD

    eng = _engines()["cnn"]
    opt = FlatSGD(eng.params, eng.grads)
    eng.new_table = torch.zeros(4)
    eng.new_list = [torch.zeros(2), 3]
    opt.second_moment = torch.zeros(4)
    eng.small.epoch_words = torch.zeros(2, dtype=torch.int32)
    assert unclassified(eng, opt) == ["FlatSGD.second_moment", "NativeCNN.new_list", "NativeCNN.new_table",
                                      "SmallLaunchState.epoch_words"]


def test_images_and_device_state_names(no_kernels):
    from wellflow.optim.flat import FlatAdam, FlatSGD

    e = _engines()
    assert images(e["mlp"]) == ["shadow", "w2t"]
    assert images(e["lstm"]) == ["WhhT", "Wp"]
    assert images(e["cnn"]) == ["WcA", "WdB", "WdF"]
    assert images(e["cnn_gemm"]) == ["shadow"]
    mlp = e["mlp"]
    mlp.shadow.zero_(), mlp.w2t.zero_()  # (torch.empty on the CPU: whatever was there)
    opt = _with_device_buffers(FlatAdam(mlp.params, mlp.grads, **mlp.fused_update_kwargs("adam")))
    opt.step_dev[:2] = torch.tensor([7.0, 1.0])
    st = device_state(mlp, opt)
    # shared tensors once, under the engine's name; step_dev is the count alone (word 1: the ticket)
    assert sorted(st) == ["grads", "m", "params", "shadow", "step_dev", "v", "w2t"]
    assert st["step_dev"].tolist() == [7.0]
    st["params"].add_(1.0)  # clones
    assert float(mlp.params.abs().max()) == 0.0
    cnn = e["cnn"]
    cnn.WcA.zero_(), cnn.WdF.zero_(), cnn.WdB.zero_()
    st = device_state(cnn, _with_device_buffers(FlatSGD(cnn.params, cnn.grads)))
    assert sorted(st) == ["WcA", "WdB", "WdF", "grads", "params", "rng", "step_dev", "vel"]


def test_compare_states_reads_bit_patterns():
    a = {"w": torch.tensor([1.0, 2.0, 3.0]), "img": torch.tensor([1.0, -2.0]).bfloat16(),
         "n": torch.tensor([5], dtype=torch.int64)}
    same = {k: v.clone() for k, v in a.items()}
    assert compare_states(a, same) == []
    # one flipped low bit, in fp32 and in bf16
    b = {k: v.clone() for k, v in a.items()}
    b["w"].view(torch.int32)[1] ^= 1
    assert b["w"][1].item() != 2.0 and abs(b["w"][1].item() - 2.0) < 1e-6
    assert compare_states(a, b) == ["w"]
    b["img"].view(torch.int16)[0] ^= 1
    assert compare_states(a, b) == ["img", "w"]
    # an integer counter
    c = {k: v.clone() for k, v in a.items()}
    c["n"] += 1
    assert compare_states(a, c) == ["n"]


def test_compare_states_nan_and_signed_zero():
    nan = torch.tensor([float("nan"), 1.0])
    assert compare_states({"x": nan}, {"x": nan.clone()}) == []  # the same NaN is the same state
    other = nan.clone()
    other.view(torch.int32)[0] ^= 1  # another NaN payload
    assert torch.isnan(other[0]) and compare_states({"x": nan}, {"x": other}) == ["x"]
    assert compare_states({"x": torch.tensor([0.0])}, {"x": torch.tensor([-0.0])}) == ["x"]
    z = torch.tensor([0.0, -0.0]).bfloat16()
    assert compare_states({"x": z}, {"x": z.clone()}) == []
    assert compare_states({"x": z}, {"x": z.flip(0)}) == ["x"]


def test_compare_states_missing_key_shape_and_dtype():
    a = {"p": torch.zeros(4), "m": torch.zeros(4)}
    assert compare_states(a, {"p": torch.zeros(4)}) == ["m"]
    assert compare_states({"p": torch.zeros(4)}, a) == ["m"]
    assert compare_states(a, {"p": torch.zeros(5), "m": torch.zeros(4)}) == ["p"]
    assert compare_states(a, {"p": torch.zeros(4).bfloat16(), "m": torch.zeros(4)}) == ["p"]
    assert compare_states(a, {"p": torch.zeros(2, 2), "m": torch.zeros(4)}) == ["p"]
