"""Does a trained generation beat an untrained one?  Trains N generations from a fresh net with AlphaSnakeZeroTrainer at
train.py's settings (11x11, 4 snakes, 256 self-play games, depth 8, breadth 128, lr 1e-4, decay 0.98), then lets the
reference's own judge decide on the device arena (snake_engine.arena.Arena.test_pit: test_pit.py's 1 v 3 in both seatings
and its two-snake duel): generation N against generation 0 and against generation N/2, with 300 and with 4 096 games.
Every judged generation (N, N/2 and 0) also meets the scripted opponent (snake_engine.arena.Scripted with the whole policy) in
the same three seatings: the one opponent whose strength does not move from run to run, so these lines can be compared with last
week's.  (Since the scripted opponent was added this script has not been run: profiles/learning_run.log has no such line yet.)

    python tools/learning_run.py [N = 30] [--out profiles] [--games 300 4096] [--seed 1] [--search BREADTH] [--league M]

--search BREADTH plays the final pits both ways: with greedy sides as above, then with both nets moving by search
(snake_engine.arena.Searcher, depth as in training, the given breadth).

--league M adds one league match (snake_engine.league.round_robin, duels, the first game count) among M generations spread
evenly from 0 to N: the cross table, the scores and the Bradley-Terry ratings, beside the pit lines.  Together with
--search BREADTH the same round robin is played once more with every seat moving by search (League.play_search).

Writes <out>/learning_log.csv (the trainer's log.csv) and <out>/learning_run.log: seconds per generation, the range-guard
widenings of self-play, the fit's mode, and the pit lines in the reference's wording with a 95 % Wilson interval on every
rate (chance is 0.25 for the lone snake of a 1 v 3 between equals, 0.5 for the duel).  Nothing is asserted: the numbers are
the result."""
import argparse
import math
import os
import random
import shutil
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "alphasnake-zero_amd")
for p in (REPO, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)


def wilson(k, n, z=1.96):
    if n == 0:
        return 0.0, 1.0
    ph, d = k / n, 1 + z * z / n
    c, h = ph + z * z / (2 * n), z * math.sqrt(ph * (1 - ph) / n + z * z / (4 * n * n))
    return (c - h) / d, (c + h) / d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("generations", nargs="?", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles"))
    ap.add_argument("--games", nargs="*", type=int, default=[300, 4096])
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--search", type=int, default=None, metavar="BREADTH")
    ap.add_argument("--league", type=int, default=None, metavar="M")
    a = ap.parse_args()
    N, out = a.generations, os.path.abspath(a.out)
    os.makedirs(out, exist_ok=True)
    import numpy as np
    import torch
    import train as train_script
    from snake_engine.arena import Arena, Scripted
    from utils import trainer_torch
    from utils.alpha_nnet import AlphaNNet
    from utils.alpha_snake_zero_trainer import AlphaSnakeZeroTrainer
    from utils.mp_game_runner import MPGameRunner
    random.seed(a.seed); np.random.seed(a.seed)
    MPGameRunner.verbose = False
    s = train_script.SETTINGS
    log_path = os.path.join(out, "learning_run.log")
    open(log_path, "w").close()

    def say(text):                                  # the log grows as the run goes: a run that is cut short leaves what it had
        print(text, flush=True)
        with open(log_path, "a") as f:
            f.write(text + "\n")

    class Timed(AlphaSnakeZeroTrainer):
        marks, trips, records = [], 0, []

        def _self_play(self, nnet, iteration):
            Timed.marks.append(time.time())
            if iteration:
                shutil.copyfile("log.csv", os.path.join(out, "learning_log.csv"))
                say(f"generation {iteration - 1}: {Timed.marks[-1] - Timed.marks[-2]:.1f} s")
            alice, runner = super()._self_play(nnet, iteration)
            Timed.trips += int(getattr(getattr(nnet, "_qnet", None), "guard_trips", 0))
            Timed.records.append(len(alice.records))
            return alice, runner

    work = tempfile.mkdtemp(prefix="learning_run_")
    here = os.getcwd()
    os.chdir(work)
    try:
        os.makedirs("models")
        h, w = s["game_board_height"], s["game_board_width"]
        net0 = AlphaNNet(input_shape=(2 * h - 1, 2 * w - 1, 3))
        net0.save("gen0")
        say(f"learning_run: {N} generations, settings {s}, seed {a.seed}, SNK_TRAIN_DATA={os.environ.get('SNK_TRAIN_DATA') or 'host'}, "
            f"{torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName}), ROCm / HIP {torch.version.hip}")
        trainer = Timed(s["self_play_games"], s["max_MCTS_depth"], s["max_MCTS_breadth"], s["initial_learning_rate"],
                        s["learning_rate_decay"], h, w, s["number_of_snakes"], None)
        t0 = time.time()
        trainer.train(net0, name="gen", iteration=0, max_iterations=N)
        torch.cuda.synchronize()
        Timed.marks.append(time.time())
        secs = [b - c for b, c in zip(Timed.marks[1:], Timed.marks[:-1])]
        say(f"training: {time.time() - t0:.1f} s in all; seconds per generation: " + " ".join(f"{x:.1f}" for x in secs))
        say("records per generation: " + " ".join(str(r) for r in Timed.records))
        say(f"range-guard widenings during self-play: {Timed.trips}; fit.last_mode: {trainer_torch.fit.last_mode}")
        shutil.copyfile("log.csv", os.path.join(out, "learning_log.csv"))

        def load(g):
            return AlphaNNet(model_name=f"models/gen{g}.h5")
        new = load(N)
        for old_gen in sorted({0, N // 2}):
            if old_gen == N:
                continue
            old = load(old_gen)
            names = (f"gen{N}", f"gen{old_gen}")
            judges = [("", None)] + ([(f" search breadth {a.search}", dict(breadth=a.search, depth=s["max_MCTS_depth"]))] if a.search else [])
            for games in a.games:
                for tag, search in judges:
                    t1 = time.time()
                    r = Arena.test_pit(new, old, games, seed=1000 + games, search=search)
                    dt = time.time() - t1
                    for me, key in ((0, "1v3_alice"), (1, "1v3_bob")):
                        win, draw = r[key]
                        lo, hi = wilson(round(win * games), games)
                        say(f"[{games} games{tag}] 1v3 Win Rate of {names[me]} {win} Draw Rate = {draw}   (95 % interval {lo:.3f}-{hi:.3f}, chance 0.25)")
                    for me in (0, 1):
                        win = r["2v2"][me]
                        lo, hi = wilson(round(win * games), games)
                        say(f"[{games} games{tag}] 2v2 Win Rate of {names[me]} {win}   (95 % interval {lo:.3f}-{hi:.3f}, chance 0.5)")
                    say(f"[{games} games{tag}] Competing time {dt:.1f}")
        for gen in sorted({0, N // 2, N}, reverse=True):          # the fixed yardstick: each judged generation against the script
            net = load(gen)
            for games in a.games:
                t1 = time.time()
                r = Arena.test_pit(net, Scripted(), games, seed=3000 + games)
                for (win, draw), seating, chance in ((r["1v3_alice"], f"gen{gen} alone against three of the script", 0.25),
                                                     (r["1v3_bob"], f"the script alone against three of gen{gen}", 0.25)):
                    lo, hi = wilson(round(win * games), games)
                    say(f"[{games} games, script] 1v3 Win Rate of the lone snake, {seating}: {win} Draw Rate = {draw}   "
                        f"(95 % interval {lo:.3f}-{hi:.3f}, chance {chance})")
                for who, win in zip((f"gen{gen}", "the script"), r["2v2"]):
                    lo, hi = wilson(round(win * games), games)
                    say(f"[{games} games, script] 2v2 Win Rate of {who} {win}   (95 % interval {lo:.3f}-{hi:.3f})")
                say(f"[{games} games, script] Competing time {time.time() - t1:.1f}")
        if a.league:
            from league import format_table                      # tools/league.py
            from snake_engine.league import round_robin
            M = max(2, min(a.league, N + 1, 16))
            gens = sorted({round(i * N / (M - 1)) for i in range(M)})
            games = a.games[0] if a.games else 300
            judges = [("", None)] + ([(f", search breadth {a.search}", dict(breadth=a.search, depth=s["max_MCTS_depth"]))] if a.search else [])
            for tag, search in judges:
                t1 = time.time()
                t, r = round_robin([load(g) for g in gens], games=games, seats="duel", height=h, width=w, seed=2000 + games, search=search)
                say(f"[league, {games} games per ordered pair, duels{tag}] generations {gens}: wins of the row's net over the column's / "
                    f"draws, score, rating (generation {gens[0]} = 0); {time.time() - t1:.1f} s")
                for line in format_table([f"gen{g}" for g in gens], t, r):
                    say(line)
    finally:
        os.chdir(here)
        shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
