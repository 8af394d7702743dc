"""The host-side half of SNK_TRAIN_DATA=device, checkable without a GPU: fit() from torch tensors, the new symbol's declaration
and binding, the seedable shared-seed stream of the multi-rank sample split, and the device form of the multi-rank mirror step."""
import os
import re

import numpy as np
import torch

from conftest import REPO


def _tiny_problem(seed=0, n=12, hw=5):
    from snake_engine.net import glorot_uniform_weights
    rng = np.random.RandomState(seed)
    ws = glorot_uniform_weights((hw, hw, 3), blocks=1, seed=seed)
    for k in (1, 6, 11, 16):                    # non-trivial batch-norm parameters
        ws[k] = (1.0 + 0.2 * rng.randn(*ws[k].shape)).astype(np.float32)
        ws[k + 1] = (0.1 * rng.randn(*ws[k].shape)).astype(np.float32)
    X = rng.rand(n, hw, hw, 3).astype(np.float32)
    Y = np.tanh(rng.randn(n, 3)).astype(np.float32) * 0.7
    return ws, X, Y


def test_fit_from_torch_tensors_equals_fit_from_arrays():
    """the CPU autograd path in float64: the same weights, bit for bit, whether X and Y arrive as arrays or as tensors -- also
    when the seed is fit's own draw from the global NumPy stream (the tensor branch must leave that draw where it was)"""
    from utils import trainer_torch
    ws, X, Y = _tiny_problem()
    kw = dict(epochs=3, batch_size=5, lr_schedule=([2, 4], [1e-2, 2.5e-3, 6e-4]), device=torch.device("cpu"), verbose=False,
              dtype=torch.float64)
    for seed in (3, None):
        np.random.seed(9)
        a = trainer_torch.fit(ws, (5, 5, 3), X, Y, seed=seed, **kw)
        after_a = np.random.randint(1 << 31)
        np.random.seed(9)
        b = trainer_torch.fit(ws, (5, 5, 3), torch.as_tensor(X), torch.as_tensor(Y), seed=seed, **kw)
        after_b = np.random.randint(1 << 31)
        assert trainer_torch.fit.last_mode == "autograd" and after_a == after_b
        assert len(a) == len(b) == len(ws)
        for i, (p, q) in enumerate(zip(a, b)):
            assert p.dtype == q.dtype and p.tobytes() == q.tobytes(), f"weight array {i}"
        assert max(np.abs(p - np.asarray(w, np.float64)).max() for p, w in zip(a, ws)) > 1e-3      # it did move
    # a non-contiguous tensor view is taken as it is (fit makes it contiguous)
    Xt = torch.as_tensor(np.ascontiguousarray(X.transpose(0, 2, 1, 3))).permute(0, 2, 1, 3)
    assert not Xt.is_contiguous()
    c = trainer_torch.fit(ws, (5, 5, 3), Xt, torch.as_tensor(Y), seed=3, **kw)
    d = trainer_torch.fit(ws, (5, 5, 3), X, Y, seed=3, **kw)
    assert all(p.tobytes() == q.tobytes() for p, q in zip(c, d))


def test_observe_mirror_is_declared_and_bound_and_the_abi_version_stays():
    from snake_engine import _lib
    header = open(os.path.join(REPO, "include", "snake_engine.h")).read()
    decl = re.search(r"int snk_engine_observe_mirror\(([^;]*)\);", header)
    assert decl, "include/snake_engine.h declares snk_engine_observe_mirror"
    args = [a.strip() for a in " ".join(decl.group(1).split()).split(",")]
    assert args == ["const snk_engine *e", "const int32_t *d_pairs", "const int32_t *d_index", "const uint8_t *d_mirror", "int m",
                    "int layout", "float *d_planes", "void *stream"]
    restype, argtypes = _lib.PROTOTYPES["snk_engine_observe_mirror"]
    assert len(argtypes) == len(args)
    assert int(re.search(r"#define SNK_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION == 113
    L = _lib.lib()                                           # the built library exports it and binds
    assert L.snk_engine_observe_mirror.argtypes is not None and L.snk_version() == 113


def test_dist_seed_makes_the_shared_seed_repeatable():
    from snake_engine import dist
    saved = dist._seed_stream
    try:
        dist.seed(7)
        _, a = dist.gather_counts(100)
        _, a2 = dist.gather_counts(100)
        dist.seed(7)
        _, b = dist.gather_counts(100)
        _, b2 = dist.gather_counts(100)
        assert (a, a2) == (b, b2) and a != a2
        # ... and with it the hypergeometric top-up of a short rank's share
        assert dist.share_counts([10, 500, 500, 500], 1200, a) == dist.share_counts([10, 500, 500, 500], 1200, b)
        dist.seed(8)
        assert dist.gather_counts(100)[1] != a
        # the default: two fresh streams, seeded from OS entropy, differ (31-bit draws, four of them)
        fresh = [np.random.Generator(np.random.PCG64()) for _ in range(2)]
        assert [int(g.integers(1 << 31)) for g in [fresh[0]] * 4] != [int(g.integers(1 << 31)) for g in [fresh[1]] * 4]
    finally:
        dist._seed_stream = saved


def test_dist_seed_leaves_the_global_generators_alone():
    import random
    from snake_engine import dist
    saved = dist._seed_stream
    try:
        np.random.seed(1)
        random.seed(1)
        want = (np.random.randint(1 << 31), random.random())
        np.random.seed(1)
        random.seed(1)
        dist.seed(3)
        dist.gather_counts(5)
        assert (np.random.randint(1 << 31), random.random()) == want
    finally:
        dist._seed_stream = saved


def test_multi_rank_mirror_step_on_a_gathered_tensor_equals_the_host_lists():
    """what _collect's several-rank branch does after the all-gather, without torch.distributed: the device form appends
    torch.flip of the gathered tensors, the host form turns them into lists and appends np.flip"""
    from utils.alpha_snake_zero_trainer import AlphaSnakeZeroTrainer
    rng = np.random.RandomState(2)
    Xg = torch.as_tensor(rng.rand(10, 13, 13, 3).astype(np.float32))
    Vg = torch.as_tensor(np.tanh(rng.randn(10, 3)).astype(np.float32))
    t = AlphaSnakeZeroTrainer(8, 2, 8, 1e-3, 0.98, 7, 7, 2)
    X, V = list(Xg.cpu().numpy()), list(Vg.cpu().numpy())
    X += t.mirror_states(X)
    V += t.mirror_values(V)
    Xd, Vd = t.mirror_device(Xg, Vg)
    assert torch.is_tensor(Xd) and Xd.device == Xg.device and Xd.dtype == torch.float32 and Xd.is_contiguous()
    assert tuple(Xd.shape) == (20, 13, 13, 3) and tuple(Vd.shape) == (20, 3)
    assert Xd.numpy().tobytes() == np.array(X, np.float32).tobytes()
    assert Vd.numpy().tobytes() == np.array(V, np.float32).tobytes()
    # no rows: both forms give an empty set
    Xe, Ve = t.mirror_device(Xg[:0], Vg[:0])
    assert tuple(Xe.shape) == (0, 13, 13, 3) and tuple(Ve.shape) == (0, 3) and t.mirror_states([]) == []


def test_the_switch_is_read_at_construction(monkeypatch):
    import pytest
    from utils.alpha_snake_zero_trainer import AlphaSnakeZeroTrainer
    monkeypatch.delenv("SNK_TRAIN_DATA", raising=False)
    assert AlphaSnakeZeroTrainer(8, 2, 8, 1e-3, 0.98).train_data == "host"
    monkeypatch.setenv("SNK_TRAIN_DATA", "")
    assert AlphaSnakeZeroTrainer(8, 2, 8, 1e-3, 0.98).train_data == "host"
    monkeypatch.setenv("SNK_TRAIN_DATA", "device")
    t = AlphaSnakeZeroTrainer(8, 2, 8, 1e-3, 0.98)
    monkeypatch.delenv("SNK_TRAIN_DATA")
    assert t.train_data == "device"
    monkeypatch.setenv("SNK_TRAIN_DATA", "hbm")
    with pytest.raises(ValueError, match="SNK_TRAIN_DATA"):
        AlphaSnakeZeroTrainer(8, 2, 8, 1e-3, 0.98)
