"""The scripted opponent's cost (snake_engine.arena.Scripted, snk_pit_script_values) beside what it replaces for its seats.

    python tools/script_time.py [--reps 20] [--pairs 3] [--games 300 4096] [--blocks 4] [--log profiles/script_time.log]
                                [--forms script look deep play terr net lookt deep2t playt lookth40 ...]

kernel: HIP-event time of one snk_pit_script_values launch over the first 16 384 alive rows of 11x11x4 boards and the first 4 096
of 19x19x8 boards, both taken from games the script itself has played for 20 turns (mid-game bodies, some snakes dead), beside the
observe launch plus a --blocks-block forward over the same rows; medians of --reps launches after one that is not timed.  Beside it
one snk_pit_look_values call (snake_engine.arena.Lookahead: its plan, the clone, step and script launches on the sub-engine and
the reduce) over the same rows, one Deep(depth=2) and one Playout() with its defaults (snake_engine.arena.Playout,
snk_pit_playout_values: 3 + 3 * horizon + 1 launches a call), and one snk_pit_territory_values launch (snake_engine.arena.Territory:
one kernel, no sub-engine).
match: ms per turn of Arena.match(Scripted, Scripted) beside Lookahead against Lookahead, Deep against Deep, Playout against
Playout, Territory against Territory and greedy net against greedy net (1 v 3,
11x11), alternating inside this one process, --pairs times; a host clock around a match that ends in a device synchronise.
--forms: the players that are timed, all six by default; script is always among them (the others are given beside it).  The
lookahead line needs look, the deep and playout lines need look too (they are given as multiples of it).  deep2 is deep.  A name
of tools/leaf_names.py (lookt, deep2t, playt, lookth40, ...: that search with territory at the leaf) adds one line per board: one
call of the _leaf entry point (snk_pit_look_values_leaf, ...) by events beside the plain call over the same rows, timed next to
it, and the player against itself among the matches."""
import argparse
import os
import statistics
import sys
import time

import leaf_names

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "alphasnake-zero_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


FORMS = ("script", "look", "deep", "play", "terr", "net")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--games", type=int, nargs="*", default=[300, 4096])
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--log", default=None)
    ap.add_argument("--forms", nargs="+", default=list(FORMS),
                    type=lambda v: v if v in FORMS + ("deep2",) or leaf_names.parse(v) is not None
                    else ap.error(f"--forms {v}: one of {' '.join(FORMS)}, deep2, or a search with t or thN behind it (lookt, deep2th40)"))
    a = ap.parse_args()
    leaf_forms = [v for v in dict.fromkeys(a.forms) if leaf_names.parse(v) is not None]
    forms = {"deep" if v == "deep2" else v for v in a.forms if v not in leaf_forms} | {"script"}
    if forms & {"deep", "play"} and "look" not in forms:
        ap.error("--forms deep and play are given as multiples of look: name look as well")
    import torch
    from snake_engine import Engine
    from snake_engine._lib import check
    from snake_engine import arena as arena_mod
    from snake_engine.arena import Arena, Deep, Lookahead, Playout, Scripted, Territory
    from snake_engine.engine import _ptr, _stream
    from snake_engine.net import glorot_uniform_weights
    from utils.alpha_nnet import AlphaNNet

    def say(s):
        print(s, flush=True)
        if a.log:
            os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
            with open(a.log, "a") as f:
                f.write(s + "\n")

    prop = torch.cuda.get_device_properties(0)
    say(f"script_time: {torch.cuda.get_device_name(0)} ({prop.gcnArchName}, {prop.multi_processor_count} CUs), ROCm / HIP "
        f"{torch.version.hip}, torch {torch.__version__}")
    script, look, deep, play, terr = Scripted(), Lookahead(), Deep(depth=2), Playout(), Territory()

    def plain_of(name):
        """the player of a leaf name without its leaf"""
        kind, kw, _ = leaf_names.parse(name)
        return {"look": Lookahead, "deep": Deep, "play": Playout}[kind](**kw)
    leaf_sides = {name: (plain_of(name), leaf_names.player(name, arena_mod)) for name in leaf_forms}

    def events(fn):
        fn()
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1) * 1e3)
        return statistics.median(ms), min(ms), max(ms)

    for hw, S, n, rows in ((11, 4, 6144, 16384), (19, 8, 1024, 4096)):
        eng = Engine(n, hw, hw, S, 1, 0.15, seed=3)
        eng.reset()
        moves = eng.new((n, S), torch.uint8)
        for _ in range(20):                          # the script plays every seat: mid-game boards
            pairs, cnt = eng.ids()
            m = int(cnt.item())
            check(eng.L.snk_pit_moves(_ptr(script.q_rows(eng, pairs[:m])), _ptr(pairs), m, n, S, _ptr(moves), _stream()))
            eng.step(moves)
        pairs, cnt = eng.ids()
        m = int(cnt.item())
        if m < rows:
            raise SystemExit(f"{hw}x{hw}x{S}: only {m} alive rows of {rows} after 20 turns")
        pairs = pairs[:rows].contiguous()
        k = events(lambda: script.q_rows(eng, pairs))
        if "net" in forms:
            net = AlphaNNet(input_shape=(2 * hw - 1, 2 * hw - 1, 3), _weights=glorot_uniform_weights((2 * hw - 1, 2 * hw - 1, 3), a.blocks, seed=1))

            def forward():
                planes, mask, _ = eng.observe_all(pairs, want_key=False)
                return net.v_device(planes, mask)
            forward()
            o = events(lambda: eng.observe_all(pairs, want_key=False))
            f = events(forward)
            say(f"kernel: {hw}x{hw}x{S}, {rows} rows of {n} games after 20 scripted turns ({m} alive rows): snk_pit_script_values "
                f"{k[0]:.1f} us (min {k[1]:.1f}, max {k[2]:.1f}); observe alone {o[0]:.1f} us; observe + {a.blocks}-block forward "
                f"{f[0]:.1f} us (min {f[1]:.1f}, max {f[2]:.1f}); ratio {f[0] / k[0]:.1f}x")
        else:
            say(f"kernel: {hw}x{hw}x{S}, {rows} rows of {n} games after 20 scripted turns ({m} alive rows): snk_pit_script_values "
                f"{k[0]:.1f} us (min {k[1]:.1f}, max {k[2]:.1f})")
        if "look" in forms:
            look.q_rows(eng, pairs)                  # the sub-engine and the scratch are made outside the timing
            la = events(lambda: look.q_rows(eng, pairs))
            say(f"kernel: {hw}x{hw}x{S}, the same {rows} rows: snk_pit_look_values {la[0]:.1f} us (min {la[1]:.1f}, max {la[2]:.1f}), "
                f"{la[0] / k[0]:.1f}x snk_pit_script_values; sub-engine of {look._sub.n_slots} slots")
        if "deep" in forms:
            deep.q_rows(eng, pairs)                  # the sub-engines and the scratch are made outside the timing
            d = events(lambda: deep.q_rows(eng, pairs))
            say(f"kernel: {hw}x{hw}x{S}, the same {rows} rows: Deep(depth=2), snk_pit_deep_values in chunks of {deep._subs[0].n_slots // 81} "
                f"rows, {d[0]:.1f} us (min {d[1]:.1f}, max {d[2]:.1f}), {d[0] / la[0]:.1f}x snk_pit_look_values; sub-engines of "
                f"{[sub.n_slots for sub in deep._subs]} slots, {sum(sub.n_slots * sub.slot_bytes for sub in deep._subs) / 2 ** 20:.0f} MiB")
        if "play" in forms:
            play.q_rows(eng, pairs)                  # the sub-engine and the scratch are made outside the timing
            pl = events(lambda: play.q_rows(eng, pairs))
            per = max(arena_mod.PLAYOUT_SLOT_BUDGET // (3 * play.playouts), 1)
            say(f"kernel: {hw}x{hw}x{S}, the same {rows} rows: Playout() ({play.playouts} playouts of {play.horizon} ticks), "
                f"snk_pit_playout_values in {(rows + per - 1) // per} calls of at most {per} rows, {pl[0]:.1f} us (min {pl[1]:.1f}, max {pl[2]:.1f}), "
                f"{pl[0] / la[0]:.1f}x snk_pit_look_values, {pl[0] / k[0]:.1f}x snk_pit_script_values; sub-engine of {play._sub.n_slots} slots, "
                f"{play._sub.n_slots * play._sub.slot_bytes / 2 ** 20:.0f} MiB")
        if "terr" in forms:
            k2 = events(lambda: script.q_rows(eng, pairs))       # the script once more, next to the launch it is compared with
            te = events(lambda: terr.q_rows(eng, pairs))
            say(f"kernel: {hw}x{hw}x{S}, the same {rows} rows: snk_pit_territory_values {te[0]:.1f} us (min {te[1]:.1f}, max {te[2]:.1f}), "
                f"{te[0] / k2[0]:.1f}x snk_pit_script_values ({k2[0]:.1f} us, min {k2[1]:.1f}, max {k2[2]:.1f}, timed beside it); one launch, "
                f"no sub-engine")
        for name, (plain, leafed) in leaf_sides.items():
            plain.q_rows(eng, pairs)                 # the sub-engines and the scratch are made outside the timing
            leafed.q_rows(eng, pairs)
            pe = events(lambda: plain.q_rows(eng, pairs))
            le = events(lambda: leafed.q_rows(eng, pairs))
            say(f"kernel: {hw}x{hw}x{S}, the same {rows} rows: {name} ({type(leafed).__name__} with leaf Territory(hungry={leafed.leaf.hungry}), "
                f"the _leaf entry point) {le[0]:.1f} us (min {le[1]:.1f}, max {le[2]:.1f}), {le[0] / pe[0]:.3f}x the plain call "
                f"({pe[0]:.1f} us, min {pe[1]:.1f}, max {pe[2]:.1f}, timed beside it)")

    sides_of = {"script v script": (script, Scripted())}
    Arena(11, 11, 4, 1, 64, 99).match(script, Scripted(), 1)           # first launches settle outside the timing
    if "look" in forms:
        sides_of["look v look"] = (Lookahead(), Lookahead())
    if "deep" in forms:
        sides_of["deep v deep"] = (Deep(depth=2), Deep(depth=2))
    if "play" in forms:
        sides_of["play v play"] = (Playout(), Playout(seed=1))
    if "terr" in forms:
        sides_of["terr v terr"] = (terr, Territory())
        Arena(11, 11, 4, 1, 64, 99).match(terr, Territory(), 1)
    for name in leaf_forms:
        sides_of[f"{name} v {name}"] = (leaf_names.player(name, arena_mod), leaf_names.player(name, arena_mod))
    if "net" in forms:
        nets = [AlphaNNet(input_shape=(21, 21, 3), _weights=glorot_uniform_weights((21, 21, 3), a.blocks, seed=s)) for s in (1, 2)]
        Arena(11, 11, 4, 1, 64, 99).match(nets[0], nets[1], 1)         # plans and range-guard scales settle outside the timing
        sides_of["net v net"] = nets
    for n in a.games:
        if "look" in forms:                                            # their sub-engines grow to this size outside the timing
            Arena(11, 11, 4, 1, n, 99).match(*sides_of["look v look"], 1)
        per = {name: [] for name in sides_of}
        for k in range(a.pairs):
            for name, sides in sides_of.items():
                arena = Arena(11, 11, 4, 1, n, seed=7)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res = arena.match(sides[0], sides[1], 1)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                per[name].append(dt / res.turns * 1e3)
                say(f"match: games {n:5d} pair {k} {name}: {res.turns:4d} turns, {dt:7.3f} s, {dt / res.turns * 1e3:7.3f} ms per turn, "
                    f"wins {res.wins_a}-{res.wins_b}, draws {res.draws}")
        med = {name: statistics.median(v) for name, v in per.items()}
        s = med["script v script"]
        say(f"match: games {n:5d} median ms per turn: " + ", ".join(f"{name} {v:.3f}" for name, v in med.items()) + "; over script v script: "
            + ", ".join(f"{name.split()[0]} {v / s:.2f}x" for name, v in med.items() if name != "script v script"))


if __name__ == "__main__":
    main()
