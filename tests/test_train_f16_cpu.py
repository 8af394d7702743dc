"""CPU checks of the training step's single-pass f16 mode (TrainStep(conv="f16"), SNK_TRAIN_CONV=f16): the new entry points are
declared, exported and bound (tests/test_abi_cpu.py compares the header with the prototypes; this file names the symbols the mode
needs), the ABI version stays, and the switch changes nothing where no GPU runs the kernels."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import REPO

F16_SYMBOLS = ["snk_conv3x3_f16_stats", "snk_conv3x3_f16_stats_deferred", "snk_conv3x3_f16_igrad_stats",
               "snk_conv3x3_f16_igrad_stats_deferred", "snk_conv3x3_f16_igrad_stats_masked_res",
               "snk_conv3x3_f16_igrad_stats_masked_res_deferred", "snk_conv3x3_wgrad_f16", "snk_conv3x3_wgrad_f16_deferred"]


def test_every_f16_entry_point_is_declared_exported_and_bound_like_its_split_namesake():
    import snake_engine
    from snake_engine import _lib
    L = snake_engine.lib()
    header = open(os.path.join(REPO, "include", "snake_engine.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in F16_SYMBOLS:
        split = name.replace("_f16", "_f16s", 1)
        assert re.search(r"\bint %s\s*\(" % name, header), f"include/snake_engine.h does not declare {name}"
        assert hasattr(L, name), f"libsnake_engine.so lacks {name}"
        assert _lib.PROTOTYPES[name] == _lib.PROTOTYPES[split], f"{name} and {split} take different argument lists"
        # ... in the header too: the two declarations differ in the name only
        decl = lambda n: re.sub(r"\s+", " ", re.search(r"\bint %s\s*\((.*?)\);" % n, header, flags=re.S).group(1))
        assert decl(name) == decl(split), name
    assert _lib.ABI_VERSION == 113 and L.snk_version() == 113


def _tiny():
    from snake_engine.net import glorot_uniform_weights
    rng = np.random.RandomState(0)
    ws = glorot_uniform_weights((5, 5, 3), blocks=1, seed=0)
    X = rng.rand(12, 5, 5, 3).astype(np.float32)
    Y = np.tanh(rng.randn(12, 3)).astype(np.float32)
    return ws, X, Y


def test_without_a_gpu_fit_does_under_f16_what_it_does_under_the_default(monkeypatch):
    """the mode selects kernels; where fit runs on PyTorch's operators (a CPU device) it changes nothing, not a bit"""
    from utils import trainer_torch
    ws, X, Y = _tiny()
    outs = {}
    for f16 in (False, True):
        monkeypatch.setattr(trainer_torch, "_CONV_F16", f16)
        outs[f16] = trainer_torch.fit(ws, (5, 5, 3), X, Y, 2, 4, ([100], [1e-3, 0.0]), device=torch.device("cpu"), seed=3, verbose=False)
        assert trainer_torch.fit.last_mode == "autograd"
    assert all(np.array_equal(a, b) for a, b in zip(outs[False], outs[True]))


def test_f16_mode_and_the_slab_weight_gradient_do_not_combine(monkeypatch):
    from snake_engine import train_step
    from utils import trainer_torch
    ws, X, Y = _tiny()
    monkeypatch.setenv("SNK_WGRAD", "slabs")
    monkeypatch.setattr(trainer_torch, "_CONV_F16", True)
    with pytest.raises(ValueError, match="SNK_WGRAD=slabs"):
        trainer_torch.fit(ws, (5, 5, 3), X, Y, 1, 4, ([100], [1e-3, 0.0]), device=torch.device("cpu"), seed=3, verbose=False)
    with pytest.raises(ValueError, match="SNK_WGRAD=slabs"):
        train_step.TrainStep(ws, (5, 5, 3), 4, "cpu", conv="f16")
    with pytest.raises(ValueError, match="conv="):
        train_step.TrainStep(ws, (5, 5, 3), 4, "cpu", conv="bf16")
    monkeypatch.setattr(trainer_torch, "_CONV_F16", False)     # the default form keeps its slab A/B arm
    trainer_torch.fit(ws, (5, 5, 3), X, Y, 1, 4, ([100], [1e-3, 0.0]), device=torch.device("cpu"), seed=3, verbose=False)
    assert trainer_torch.fit.last_mode == "autograd"
