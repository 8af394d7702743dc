"""The --baseline names of the playout yardstick (snake_engine.arena.Playout) that tools/league.py and tools/search_pit.py accept:
play (the defaults) and playPxT (P playouts, horizon T: play8x16)."""
import re


def parse(name):
    """the keyword arguments of Playout for a --baseline name, None when the name is not one of the playout's"""
    if name == "play":
        return {}
    m = re.fullmatch(r"play(\d+)x(\d+)", name)
    return dict(playouts=int(m.group(1)), horizon=int(m.group(2))) if m else None
