"""NumPy restatement of the sub-rectangle form of the towers with 16-bit activations (SNK_CONV_ALGO=f16a / bf16 / mxfp8;
csrc/conv_split.hip: hs_rect_parts(a16 = true), k_rect_plan, k_conv3x3_f16s_rect<.., IO16 = 3>): how a rectangle is cut into
blocks, which descriptors the plan writes, which input a layer sees, and what it computes, in float64.

    constants()                               the frame constants, read from the source
    parts(hr, wr, H, W)                       Parts(parts, tiles_max, lds, staging)
    plan(boxes, grow, H, W)                   one LayerPlan(bins, count, tiles) per entry of grow
    max_blocks(n, H, W)                       n x the most parts any rectangle shape of the canvas needs
    inside(boxes, g, H, W)                    bool [n][H][W]: the box grown by g pixels, cut to the canvas
    compose(x, bg, box, g, H, W)              the input a layer sees: x on the grown box, bg elsewhere
    conv3x3(x, w)                             float64 'same' convolution, zero padding at the canvas edge
    layer(...)                                conv of the composed input, scale / shift, composed shortcut, ReLU
    one_hot_expected(...)                     the same for a kernel that is 1 at one tap from channel c to channel c: a shift

The rules, as the kernel applies them:
  rectangle   the observation's bounding box (y0, x0, y1, x1) grown by the layer's `grow` and cut to the canvas: hr x wr pixels,
              T = ceil(hr wr / 32) M tiles, cut into `parts` blocks of T // parts tiles, the first T % parts one more
  parts       the fewest, from ceil(T / 8) on, whose largest part's strip -- its rows (worst alignment of 32 tm pixels), one row above
              and one below, two halo columns -- fits an LDS buffer, (rows + 2) ((wr + 2) HS_LDP + HS_GAP16_RECT) <= HS_BUF16 bytes, and
              the staging items, min(rows + 2, H) min(wr + 2, W) <= 64 HS_NST16 pixels
  input       a pixel of x is valid inside the bounding box grown by grow_in; everywhere else on the canvas the layer reads the
              producer's constant image bg_in.  Outside the canvas it reads zero.  The shortcut: the same with grow_res / bg_res.
  output      written on the rectangle only; with bg_out every other pixel of the canvas gets bg_out's.

Like tests/conv_plan_ref.py this was written from the C++ by hand: a changed constant is followed, a rewritten rule is not.
tests/test_rect16_ref_cpu.py checks parts() against a brute-force search and the case list against what it is meant to cover;
tests/test_rect16_gpu.py holds the kernels to plan(), layer() and one_hot_expected()."""
import os
import re
from collections import namedtuple

import numpy as np

SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "alphasnake-zero_amd", "csrc", "conv_split.hip")

_NAMES = ("HS_NST16", "HS_BUF16", "HS_LDP", "HS_GAP16_RECT")

Parts = namedtuple("Parts", "parts tiles_max lds staging")     # lds / staging: that constraint rejected a smaller count
LayerPlan = namedtuple("LayerPlan", "bins count tiles")       # bins: [(largest part's tiles, sorted descriptors)], largest first

# boxes (y0, x0, y1, x1), one image each
CASES_37 = [(18, 18, 18, 18), (0, 0, 0, 0), (36, 36, 36, 36), (0, 20, 0, 20), (17, 0, 19, 0), (36, 5, 36, 30), (3, 3, 3, 34),
            (5, 16, 30, 16), (9, 9, 27, 27), (0, 0, 18, 18), (18, 18, 36, 36), (10, 2, 20, 34), (12, 1, 23, 35), (2, 12, 34, 22),
            (0, 0, 36, 36), (14, 3, 17, 33), (6, 6, 9, 13), (20, 8, 27, 15), (10, 2, 21, 32)]
CASES_9x13 = [(4, 6, 4, 6), (0, 0, 8, 12), (0, 0, 2, 3), (6, 9, 8, 12), (3, 0, 5, 12)]
GROW = (0, 1, 2, 3)                      # rectangle grows
CANVASES = [(37, 37, CASES_37), (9, 13, CASES_9x13)]


def constants(path=SRC):
    """{name: int} of the #defines the 16-bit frame's rectangle rule uses"""
    with open(path) as f:
        text = f.read()
    out = {}
    for name in _NAMES:
        m = re.findall(r"^#define\s+%s\s+(\d+)\b" % name, text, re.M)
        assert len(m) == 1, (name, m)
        out[name] = int(m[0])
    return out


_C = None


def _consts(c):
    global _C
    if c is not None:
        return c
    if _C is None:
        _C = constants()
    return _C


def strip_rows(tm, hr, wr):
    """output rows a part of tm tiles can touch: the worst alignment of 32 tm pixels in rows of wr, at most the rectangle's"""
    return min((tm * 32 + wr - 2) // wr + 1, hr)


def fits(tm, hr, wr, H, W, c=None):
    """(LDS ok, staging ok) of a part of tm tiles of an hr x wr rectangle on an H x W canvas"""
    c = _consts(c)
    rows = strip_rows(tm, hr, wr)
    lds = (rows + 2) * ((wr + 2) * c["HS_LDP"] + c["HS_GAP16_RECT"]) <= c["HS_BUF16"]
    staging = min(rows + 2, H) * min(wr + 2, W) <= 64 * c["HS_NST16"]
    return lds, staging


def parts(hr, wr, H, W, c=None):
    """hs_rect_parts(hr, wr, H, W, &tiles_max, a16 = true); parts = -1 where even one-tile parts do not fit"""
    T = (hr * wr + 31) // 32
    n = (T + 7) // 8
    lds_rej = st_rej = False
    while True:
        tm = (T + n - 1) // n
        lds, staging = fits(tm, hr, wr, H, W, c)
        if lds and staging:
            return Parts(n, tm, lds_rej, st_rej)
        lds_rej, st_rej = lds_rej or not lds, st_rej or not staging
        if tm == 1:
            return Parts(-1, 1, lds_rej, st_rej)
        n += 1


def part_tiles(hr, wr, H, W, c=None):
    """[(tile0, ntile)] of the rectangle's parts, in part order"""
    T = (hr * wr + 31) // 32
    n = parts(hr, wr, H, W, c).parts
    base, rem = T // n, T % n
    return [(k * base + min(k, rem), base + (1 if k < rem else 0)) for k in range(n)]


def rect_of(box, g, H, W):
    """(y0, x0, hr, wr) of the box grown by g, cut to the canvas"""
    y0, x0, y1, x1 = box
    ry0, rx0, ry1, rx1 = max(y0 - g, 0), max(x0 - g, 0), min(y1 + g, H - 1), min(x1 + g, W - 1)
    return ry0, rx0, ry1 - ry0 + 1, rx1 - rx0 + 1


def box_word(box):
    y0, x0, y1, x1 = box
    return y0 | x0 << 8 | y1 << 16 | x1 << 24


def plan(boxes, grow, H, W, c=None):
    """what k_rect_plan writes for each layer: descriptors (image, y0 | x0 << 8 | hr << 16 | wr << 24, tile0 | ntile << 8 |
    part << 16 | parts << 24, box word) in bins by the image's largest part, largest first (the order inside a bin is the
    atomics': here sorted); count = descriptors, tiles = M tiles they cover"""
    out = []
    for g in grow:
        bins, tiles = {}, 0
        for img, box in enumerate(boxes):
            ry0, rx0, hr, wr = rect_of(box, g, H, W)
            p = parts(hr, wr, H, W, c)
            assert p.parts > 0, (hr, wr)
            tiles += (hr * wr + 31) // 32
            rect = ry0 | rx0 << 8 | hr << 16 | wr << 24
            for k, (t0, nt) in enumerate(part_tiles(hr, wr, H, W, c)):
                bins.setdefault(p.tiles_max, []).append((img, rect, t0 | nt << 8 | k << 16 | p.parts << 24, box_word(box)))
        ordered = [(tm, sorted(bins[tm])) for tm in sorted(bins, reverse=True)]
        out.append(LayerPlan(ordered, sum(len(d) for _, d in ordered), tiles))
    return out


def max_parts(H, W, c=None):
    return max(parts(hr, wr, H, W, c).parts for hr in range(1, H + 1) for wr in range(1, W + 1))


def max_blocks(n, H, W, c=None):
    """snk_conv_rect_max_blocks_act16: descriptors (and blocks of a launch) per layer"""
    return n * max_parts(H, W, c)


def inside(boxes, g, H, W):
    """bool [n][H][W]: pixel inside the image's box grown by g (g < 0 shrinks it)"""
    yy, xx = np.arange(H)[None, :, None], np.arange(W)[None, None, :]
    b = np.asarray(boxes).reshape(-1, 4)
    y0, x0, y1, x1 = (b[:, k][:, None, None] for k in range(4))
    return (yy >= y0 - g) & (yy <= y1 + g) & (xx >= x0 - g) & (xx <= x1 + g)


def compose(x, bg, box, g, H, W):
    """x [H][W][C] on the box grown by g (cut to the canvas), bg [H][W][C] elsewhere; or a batch x [n][H][W][C] with n boxes"""
    x = np.asarray(x)
    m = inside(box, g, H, W)
    if x.ndim == 3:
        m = m[0]
    return np.where(m[..., None], x, np.asarray(bg))


def conv3x3(x, w):
    """float64 cross-correlation, 'same', zero padding: x [n][H][W][Ci], w [3][3][Ci][Co] (HWIO) -> [n][H][W][Co]"""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    n, H, W, _ = x.shape
    xp = np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0)))
    out = np.zeros((n, H, W, w.shape[3]))
    for ky in range(3):
        for kx in range(3):
            out += xp[:, ky:ky + H, kx:kx + W] @ w[ky, kx]
    return out


def layer(x, bg_in, boxes, grow_in, w, scale, shift, res=None, bg_res=None, grow_res=0, conv=None):
    """float64 [n][H][W][C]: relu(conv3x3(compose(x, bg_in, grow_in)) * scale + shift (+ compose(res, bg_res, grow_res))) on the
    whole canvas (the kernel writes the rectangle).  conv: conv3x3 of the composed input where the caller has it already
    (x, bg_in and w are not looked at then)."""
    n, H, W, _ = np.shape(x if conv is None else conv)
    if conv is None:
        conv = conv3x3(compose(x, bg_in, boxes, grow_in, H, W), w)
    out = conv * np.asarray(scale, np.float64) + np.asarray(shift, np.float64)
    if res is not None:
        out = out + compose(res, bg_res, boxes, grow_res, H, W).astype(np.float64)
    return np.maximum(out, 0.0)


def one_hot_expected(x, bg_in, boxes, grow_in, tap, res=None, bg_res=None, grow_res=0, border="zero", stale="bg"):
    """layer() for the kernel that is 1 at tap = 3 ky + kx from channel c to channel c, scale 1, shift 0:
    out[y][x] = relu(in[y + ky - 1][x + kx - 1] (+ shortcut)).  border / stale are the faults the sensitivity test plants:
    border = "bg": the pixels outside the canvas are the background's nearest instead of zero; stale = "x": the pixels outside
    the grown box are taken from x (res) itself instead of the background image."""
    x = np.asarray(x, np.float64)
    n, H, W, _ = x.shape
    bg = np.asarray(bg_in, np.float64)
    xin = x if stale == "x" else compose(x, bg, boxes, grow_in, H, W)
    pad = ((0, 0), (1, 1), (1, 1), (0, 0))
    xp = np.pad(xin, pad)
    if border == "bg":
        edge = np.pad(np.broadcast_to(bg, xin.shape), pad, mode="edge")
        ring = np.pad(np.zeros((n, H, W, 1), bool), pad, constant_values=True)
        xp = np.where(ring, edge, xp)
    ky, kx = divmod(tap, 3)
    out = xp[:, ky:ky + H, kx:kx + W]
    if res is not None:
        r = np.asarray(res, np.float64)
        out = out + (r if stale == "x" else compose(r, np.asarray(bg_res, np.float64), boxes, grow_res, H, W))
    return np.maximum(out, 0.0)
