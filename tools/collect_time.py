"""what the training set's way from the records to the fit costs per generation (trainer.py:63-83): one generation of self-play is
recorded, then two things are timed on that same recorded agent, several times over:
  collect    AlphaSnakeZeroTrainer._collect: the sample, the encoded rows and their mirror images
  fit-ready  AlphaNNet.train(X, V, epochs=0): everything train and fit do before the first optimizer step -- X and Y resident on
             the device (and the training step's buffers, the same work on both sides)
Development tool: collect_time.py [board=11] [snakes=4] [games=256] [depth=8] [breadth=128] [reps=5]
  SNK_TRAIN_DATA=device   the device form (the A/B arm): tools/ab.sh -n 3 "SNK_TRAIN_DATA=" "SNK_TRAIN_DATA=device" -- python3 tools/collect_time.py
  SNK_TREE=<path>         import the package of another checkout of this repository (an older commit's default path as the A arm)"""
import os, random, sys, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREE = os.path.abspath(os.environ.get("SNK_TREE") or REPO)
sys.path[:0] = [TREE, os.path.join(TREE, "alphasnake-zero_amd")]
import numpy as np, torch
from utils.alpha_nnet import AlphaNNet
from utils.alpha_snake_zero_trainer import AlphaSnakeZeroTrainer
from utils.mp_game_runner import MPGameRunner
from snake_engine.net import glorot_uniform_weights

arg = [int(v) for v in sys.argv[1:]] + [None] * 6
hw, snakes, games, depth, breadth, reps = (a if a is not None else d for a, d in zip(arg, (11, 4, 256, 8, 128, 5)))
shape = (2 * hw - 1, 2 * hw - 1, 3)
MPGameRunner.verbose = False
random.seed(1)
np.random.seed(1)
trainer = AlphaSnakeZeroTrainer(games, depth, breadth, 1e-4, 0.98, hw, hw, snakes)
nnet = AlphaNNet(input_shape=shape, _weights=glorot_uniform_weights(shape, 4, seed=0)).copy_and_compile()
t0 = time.time()
alice, runner = trainer._self_play(nnet, 0)
torch.cuda.synchronize()
t_play = time.time() - t0
n_records = len(alice.records)
alice.clear = lambda: None                       # the same records serve every repetition
fit_net = nnet.copy_and_compile(learning_rate=1e-4)


def once():
    torch.cuda.synchronize()
    t0 = time.time()
    X, V, bs = trainer._collect(alice)
    torch.cuda.synchronize()
    t1 = time.time()
    fit_net.train(X, V, epochs=0, batch_size=bs)
    torch.cuda.synchronize()
    t2 = time.time()
    return t1 - t0, t2 - t1, len(X)


once()                                           # warm-up: allocator, first launches
runs = [once() for _ in range(reps)]
c, f = np.median([r[0] for r in runs]), np.median([r[1] for r in runs])
mode = getattr(trainer, "train_data", "host")
print(f"{hw}x{hw}x{snakes}, {games} games: self-play {t_play:.2f} s, {n_records} records, {runs[0][2]} training rows; {reps} repetitions: "
      + " ".join(f"{a + b:.3f}" for a, b, _ in runs))
print(f"train data on the {mode}{' (tree ' + os.path.relpath(TREE, REPO) + ')' if TREE != REPO else ''}: collect {c * 1e3:.0f} ms + fit-ready {f * 1e3:.0f} ms = "
      f"{(c + f) * 1e3:.0f} ms per generation (medians of {reps}; {runs[0][2]} rows of {hw}x{hw}x{snakes})")
