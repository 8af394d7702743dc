"""SNK_TRAIN_DATA=device (run with -m gpu on an MI355X): the sampled training set as two device tensors from the records to the
fit.  The device form draws from the same generators in the same order as the host form and the observe kernel writes the mirror
images itself, so X, V and the fitted weights are compared bit for bit with the host form's lists."""
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded():
    """a short recorded self-play of a generation-0 net: 8 games of 7x7 with 2 snakes"""
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from snake_engine.net import glorot_uniform_weights
    from utils.agent import Agent
    from utils.alpha_nnet import AlphaNNet
    from utils.mp_game_runner import MPGameRunner
    MPGameRunner.verbose = False
    nnet = AlphaNNet(input_shape=(13, 13, 3), _weights=glorot_uniform_weights((13, 13, 3), 4, seed=0))
    alice = Agent(nnet, training=True, max_MCTS_depth=2, max_MCTS_breadth=8, seed=1)
    random.seed(11)
    MPGameRunner(7, 7, 2, 9, 8, seed=2).run(alice)
    assert len(alice.records) >= 16
    return alice


def _trainer(monkeypatch, mode):
    import utils.alpha_snake_zero_trainer as T
    if mode is None:
        monkeypatch.delenv("SNK_TRAIN_DATA", raising=False)
    else:
        monkeypatch.setenv("SNK_TRAIN_DATA", mode)
    return T.AlphaSnakeZeroTrainer(8, 2, 8, 1e-3, 0.98, 7, 7, 2)


def test_collect_on_the_device_equals_the_host_lists(recorded, monkeypatch):
    import torch
    alice = recorded
    monkeypatch.setattr(alice, "clear", lambda: None)
    n = len(alice.records)
    host, dev = _trainer(monkeypatch, None), _trainer(monkeypatch, "device")
    assert host.train_data == "host" and dev.train_data == "device"
    random.seed(5)
    Xh, Vh, bh = host._collect(alice)
    random.seed(5)
    Xd, Vd, bd = dev._collect(alice)
    assert isinstance(Xh, list) and isinstance(Vh, list) and len(Xh) == len(Vh) == 2 * n
    assert torch.is_tensor(Xd) and torch.is_tensor(Vd) and Xd.is_cuda and Vd.is_cuda
    assert Xd.dtype == Vd.dtype == torch.float32 and Xd.is_contiguous() and Vd.is_contiguous()
    assert tuple(Xd.shape) == (2 * n, 13, 13, 3) and tuple(Vd.shape) == (2 * n, 3)
    assert bd == bh
    assert Xd.cpu().numpy().tobytes() == np.array(Xh, np.float32).tobytes()
    assert Vd.cpu().numpy().tobytes() == np.array(Vh, np.float32).tobytes()
    # (the comparison is not vacuous: the second half really is the mirror image, and it differs from the first)
    assert torch.equal(Xd[n:], torch.flip(Xd[:n], dims=[2])) and not torch.equal(Xd[n:], Xd[:n])
    assert len(alice.records) == n                      # clear() was patched out: the fixture is unchanged


def test_unknown_switch_value_is_an_error(monkeypatch):
    with pytest.raises(ValueError, match="SNK_TRAIN_DATA"):
        _trainer(monkeypatch, "gpu")


def test_fetch_device_checks_the_flag_count(recorded):
    with pytest.raises(ValueError, match="mirror"):
        recorded.records.fetch_device([0, 1, 2], mirror=[True, False])


def test_nnet_train_from_device_tensors_equals_the_list_form():
    import torch
    from snake_engine.net import glorot_uniform_weights
    from utils import trainer_torch
    from utils.alpha_nnet import AlphaNNet
    rng = np.random.RandomState(0)
    X = rng.rand(64, 13, 13, 3).astype(np.float32)
    Y = (np.tanh(rng.randn(64, 3)) * 0.7).astype(np.float32)
    ws = glorot_uniform_weights((13, 13, 3), 4, seed=1)

    def run(x, y):
        net = AlphaNNet(input_shape=(13, 13, 3), _weights=[w.copy() for w in ws]).copy_and_compile(learning_rate=1e-3)
        np.random.seed(3)
        net.train(x, y, epochs=2, batch_size=32)
        assert trainer_torch.fit.last_mode == "kernels"
        return net.v_net.get_weights()

    from_lists = run(list(X), list(Y))
    from_device = run(torch.as_tensor(X, device="cuda"), torch.as_tensor(Y, device="cuda"))
    assert len(from_lists) == len(from_device) == len(ws)
    for i, (a, b) in enumerate(zip(from_lists, from_device)):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), f"weight array {i}"
    assert any(not np.array_equal(a, w) for a, w in zip(from_lists, ws))          # it trained


def test_the_trainer_hands_device_tensors_to_nnet_train(tmp_path, monkeypatch):
    import torch
    import utils.alpha_nnet as A
    from snake_engine.net import glorot_uniform_weights
    from utils.mp_game_runner import MPGameRunner
    MPGameRunner.verbose = False
    monkeypatch.chdir(tmp_path)
    seen = []

    def spy(self, X, Y, epochs=32, batch_size=2048):
        seen.append((X, Y, batch_size))

    monkeypatch.setattr(A.AlphaNNet, "train", spy)
    monkeypatch.setattr(A.AlphaNNet, "save", lambda self, name: None)
    trainer = _trainer(monkeypatch, "device")
    nnet = A.AlphaNNet(input_shape=(13, 13, 3), _weights=glorot_uniform_weights((13, 13, 3), 4, seed=0))
    trainer.train(nnet, "t", 0, max_iterations=1)
    assert len(seen) == 1
    X, V, bs = seen[0]
    assert torch.is_tensor(X) and torch.is_tensor(V) and X.is_cuda and V.is_cuda
    assert X.dtype == V.dtype == torch.float32
    k = X.shape[0] // 2
    assert k >= 8 and tuple(X.shape) == (2 * k, 13, 13, 3) and tuple(V.shape) == (2 * k, 3) and bs == k
    assert torch.equal(X[k:], torch.flip(X[:k], dims=[2])) and torch.equal(V[k:], torch.flip(V[:k], dims=[1]))
