"""The pit match, host loop against device loop: `MPGameRunner.run` and `MPGameRunner.run_device` on the same start boards, the
same engine seed (so the same food spawns) and the same two nets (generation-0 Glorot weights, two seeds), 11x11 with 4 snakes.

    python tools/arena_time.py [games ...] [--pairs 3] [--blocks 4] [--log profiles/arena_ab.log] [--record K | --tally]

For every game count (default 300 and 4096) the two forms alternate inside this one process, `--pairs` times; a line per
match with its turns, seconds and ms per turn, then the medians.  The winners of the two forms are compared: they play the
same match.
--record K: instead, what a replay recorder costs: Arena.match of the same two nets without a recorder and with one on the first K
games (Arena.record), alternating inside this one process on the same start boards, `--pairs` times; ms per turn of both, the
medians and the added time per turn.  The recorded match's winners and frame counts are checked against the plain one's.
--tally: the same for a tally (Arena.tally, snk_pit_tally: one more launch per turn over all games): without and with one,
alternating; the tallied match's winners and its deaths against the plain one's; then the kernel alone beside the step kernel, by
events, on the start boards (profiles/tally_ab.log)."""
import argparse
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "alphasnake-zero_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("games", nargs="*", type=int, default=[300, 4096])
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--log", default=None)
    ap.add_argument("--record", type=int, default=None, metavar="K")
    ap.add_argument("--tally", action="store_true")
    a = ap.parse_args()
    import numpy as np
    import torch
    from snake_engine.net import glorot_uniform_weights
    from utils.alpha_nnet import AlphaNNet
    from utils.pit_agent import Agent
    from utils.pit_mp_game_runner import MPGameRunner

    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    nets = [AlphaNNet(input_shape=(21, 21, 3), _weights=glorot_uniform_weights((21, 21, 3), a.blocks, seed=s)) for s in (1, 2)]
    alice, bob = Agent(nets[0]), Agent(nets[1])

    def play(form, n, start):
        np.random.seed(0)
        gr = MPGameRunner(11, 11, 4, 1, n, seed=7)
        if start is None:
            start = gr.engine.export()
        else:
            gr.engine.import_states(start)
            for g in gr.games.values():
                g._dirty()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        winners = getattr(gr, form)(alice, bob, 1)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        lengths = np.array([s.counters[5] for s in gr.engine.export()])
        return winners, int(lengths.max()), dt, start

    say(f"arena_time: 11x11, 4 snakes (1 v 3), {a.blocks}-block Glorot nets (seeds 1, 2), {a.pairs} alternating pairs per size, "
        f"{torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName}, "
        f"{torch.cuda.get_device_properties(0).multi_processor_count} CUs), ROCm / HIP {torch.version.hip}, torch {torch.__version__}")
    def write_log():
        if a.log:
            os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
            with open(a.log, "w") as f:
                f.write("\n".join(lines) + "\n")

    def match(n, start, record, tally=False):
        from snake_engine.arena import Arena
        arena = Arena(11, 11, 4, 1, n, seed=7)
        if start is None:
            start = arena.engine.export()
        else:
            arena.import_states(start)
        rep = arena.record(range(min(record, n))) if record else None
        if tally:
            rep = arena.tally()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = arena.match(nets[0], nets[1], 1)
        torch.cuda.synchronize()
        return res, time.perf_counter() - t0, start, rep

    if a.tally:
        from snake_engine._lib import check
        from snake_engine.arena import Arena
        say(f"arena_time --tally: Arena.match greedy against greedy, 11x11, 4 snakes (1 v 3), {a.blocks}-block Glorot nets, "
            f"{a.pairs} alternating pairs per size, {torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName}), "
            f"ROCm / HIP {torch.version.hip}, torch {torch.__version__}")
        match(64, None, 0)                                 # first launches, plans and range-guard scales settle outside the timing
        match(64, None, 0, True)
        for n in a.games:
            start, per = None, {"plain": [], "tallied": []}
            for k in range(a.pairs):
                won = {}
                for form in ("plain", "tallied"):
                    res, dt, start, tal = match(n, start, 0, form == "tallied")
                    won[form] = res.winners.tolist()
                    per[form].append(dt / res.turns * 1e3)
                    say(f"games {n:5d} pair {k} {form:8s}: {res.turns:4d} turns, {dt:7.3f} s, {dt / res.turns * 1e3:8.3f} ms per turn")
                    if tal is not None:
                        dead = int((tal.fate > 0).sum())
                        ok = dead + int((res.winners >= 0).sum()) <= 4 * n and int(tal.died.max()) == res.turns
                        say(f"games {n:5d} pair {k} tallied {dead} deaths, the last on the last turn and none too many: {ok}")
                say(f"games {n:5d} pair {k} winners identical: {won['plain'] == won['tallied']}")
            p, r = statistics.median(per["plain"]), statistics.median(per["tallied"])
            say(f"games {n:5d} median ms per turn: plain {p:.3f}, tallied {r:.3f}, added {(r - p) * 1e3:.1f} us per turn")
            # the kernel alone beside the step kernel, by events, on start boards (the tally changes nothing, the step is undone
            # by importing the boards again between its launches)
            arena = Arena(11, 11, 4, 1, n, seed=7)
            eng, L = arena.engine, arena.engine.L
            boards = eng.export()
            live = torch.ones((n,), dtype=torch.uint8, device="cuda")
            moves = torch.ones((n, 4), dtype=torch.uint8, device="cuda")
            out = torch.zeros((4, n, 4), dtype=torch.int32, device="cuda")
            done = torch.zeros((n,), dtype=torch.uint8, device="cuda")
            us = {"snk_pit_tally": [], "snk_engine_step_active_tape": []}
            for i in range(24):
                for name in us:
                    eng.import_states(boards)
                    torch.cuda.synchronize()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    if name == "snk_pit_tally":
                        check(L.snk_pit_tally(eng.h, live.data_ptr(), n, moves.data_ptr(), 1, out[0].data_ptr(), out[1].data_ptr(),
                                              out[2].data_ptr(), out[3].data_ptr(), torch.cuda.current_stream().cuda_stream))
                    else:
                        check(L.snk_engine_step_active_tape(eng.h, live.data_ptr(), n, moves.data_ptr(), None, done.data_ptr(), None,
                                                            torch.cuda.current_stream().cuda_stream))
                    e1.record()
                    torch.cuda.synchronize()
                    if i >= 4:
                        us[name].append(e0.elapsed_time(e1) * 1e3)
            t, st = statistics.median(us["snk_pit_tally"]), statistics.median(us["snk_engine_step_active_tape"])
            say(f"games {n:5d} one launch on the start boards, by events, median of 20: snk_pit_tally {t:.1f} us, "
                f"snk_engine_step_active_tape {st:.1f} us")
        write_log()
        return

    if a.record is not None:
        say(f"arena_time --record {a.record}: Arena.match greedy against greedy, 11x11, 4 snakes (1 v 3), {a.blocks}-block Glorot nets, "
            f"{a.pairs} alternating pairs per size, {torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName}), "
            f"ROCm / HIP {torch.version.hip}, torch {torch.__version__}")
        match(64, None, 0)                                 # first launches, plans and range-guard scales settle outside the timing
        match(64, None, min(a.record, 64))
        for n in a.games:
            start, per = None, {"plain": [], "recorded": []}
            for k in range(a.pairs):
                won = {}
                for form, record in (("plain", 0), ("recorded", a.record)):
                    res, dt, start, rep = match(n, start, record)
                    won[form] = res.winners.tolist()
                    per[form].append(dt / res.turns * 1e3)
                    say(f"games {n:5d} pair {k} {form:8s}: {res.turns:4d} turns, {dt:7.3f} s, {dt / res.turns * 1e3:8.3f} ms per turn")
                    if rep is not None:
                        ok = all(len(rep.frames(g)) == 2 * res.lengths[g] for g in rep.games.tolist())
                        say(f"games {n:5d} pair {k} recorded {len(rep.games)} games, the log doubled {rep.grown} times, frame counts right: {ok}")
                say(f"games {n:5d} pair {k} winners identical: {won['plain'] == won['recorded']}")
            p, r = statistics.median(per["plain"]), statistics.median(per["recorded"])
            say(f"games {n:5d} median ms per turn: plain {p:.3f}, recorded {r:.3f}, added {(r - p) * 1e3:.1f} us per turn")
        write_log()
        return

    _, _, _, _ = play("run_device", 64, None)              # first launches, plans and range-guard scales settle outside the timing
    _, _, _, _ = play("run", 64, None)
    for n in a.games:
        start, per = None, {"run": [], "run_device": []}
        for k in range(a.pairs):
            won = {}
            for form in ("run", "run_device"):
                won[form], turns, dt, start = play(form, n, start)
                per[form].append(dt / turns * 1e3)
                say(f"games {n:5d} pair {k} {form:10s}: {turns:4d} turns per match, {dt:7.3f} s, {dt / turns * 1e3:8.3f} ms per turn")
            same = won["run"] == won["run_device"]
            say(f"games {n:5d} pair {k} winners identical: {same}")
        h, d = statistics.median(per["run"]), statistics.median(per["run_device"])
        say(f"games {n:5d} median ms per turn: run {h:.3f}, run_device {d:.3f}, ratio {h / d:.2f}x")
    write_log()


if __name__ == "__main__":
    main()
