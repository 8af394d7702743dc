"""The --baseline names of the searching yardsticks with territory at the leaf (snake_engine.arena.Lookahead / Deep / Playout with
leaf=Territory) that tools/league.py, tools/search_pit.py and tools/script_time.py accept: the plain name with a suffix, t for
leaf = Territory() and thN for Territory(hungry=N) -- lookt, deep2t, deep3t, playt, play8x16t, lookth40, deep2th40, playth40."""
import re

import playout_names


def parse(name):
    """(kind, the keyword arguments of the player without its leaf, hungry) for a --baseline name, None when the name is not one
    of these; kind is "look", "deep" or "play" """
    m = re.fullmatch(r"(look|deep[1-4]|play(?:\d+x\d+)?)t(?:h(\d+))?", name)
    if not m or (m.group(2) is not None and int(m.group(2)) > 100):
        return None
    base, hungry = m.group(1), int(m.group(2) or 100)
    if base == "look":
        return "look", {}, hungry
    if base.startswith("deep"):
        return "deep", dict(depth=int(base[4])), hungry
    return "play", playout_names.parse(base), hungry


def player(name, arena):
    """the player of a --baseline name (arena: the module snake_engine.arena), None when the name is not one of these"""
    p = parse(name)
    if p is None:
        return None
    kind, kw, hungry = p
    return {"look": arena.Lookahead, "deep": arena.Deep, "play": arena.Playout}[kind](leaf=arena.Territory(hungry=hungry), **kw)
