"""The weight gradient of the tower's 3x3 convolution (csrc/train_wgrad.hip) on the test side: its definition in float64, and a
plain-Python restatement of which kernel body the launcher picks for a shape.

    dw_ref(x, dy)          dW[dy][dx][ci][co] = sum over n, y, x of X[n][y + dy - 1][x + dx - 1][ci] * dY[n][y][x][co], X zero-padded: the
                           first lines of train_wgrad.hip, as nine [128, rows] @ [rows, 128] products (no convolution of any library)
    body(h, w)             (NK, MAXX, WT) of the k_wgrad2_f16s instance wgrad_launch starts at default settings, or "slab" for k_wgrad_f16s
    groups(n, h, w)        how the launch cuts n images into image groups: (groups, per_group, full, short, empty)
    CASES / SLAB_SWITCH    the shapes tests/test_wgrad_stream_gpu.py runs, each with the body and the group pattern it is there for

What body() is for, and what it does not see: it restates wg2_shape, wg_shape and the dispatch chain of wgrad_launch by hand, with the
constants read from the source by regular expressions (the convention of tests/conv_plan_ref.py).  tests/test_wgrad_ref_cpu.py
asserts that CASES reaches every value body() can return at default settings and that every case runs the body and the group pattern
it claims -- so a CHANGED CONSTANT (WG_GX, the LDS limits, the staging-item limits, the two compile-time widths, WG2_GROUPS) that moves a
case to another launch line, or a parameter list that stops covering one, fails on the CPU instead of silently leaving a body
untested.  A REWRITTEN wg2_shape or dispatch chain is not seen: this file would go on stating the old one.  Whoever changes them
changes this restatement with it.  Nothing here is used by the product.
"""
import os
import re

SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "alphasnake-zero_amd", "csrc", "train_wgrad.hip")

_DEFINES = ("WG_GROUPS", "WG_GX", "WG_MAXX", "WG_MAXY", "WG2_GROUPS")


def constants(path=SRC):
    """{name: int}: the #defines, the limits inside wg2_shape / wg_shape, the default of SNK_WGRAD_NK, the compile-time widths"""
    with open(path) as f:
        text = f.read()
    out = {}
    for name in _DEFINES:
        m = re.findall(r"^#define\s+%s\s+(\d+)\b" % name, text, re.M)
        assert len(m) == 1, (name, m)
        out[name] = int(m[0])
    m = re.findall(r"s\.maxx <= (\d+) && s\.lds <= (\d+) \* 1024\)", text)
    assert len(m) == 1, m
    out["W2_MAXX"], out["W2_LDS_KB"] = int(m[0][0]), int(m[0][1])
    m = re.findall(r"s\.ny_items <= WG_MAXY \* 256 && s\.lds <= (\d+) \* 1024\)", text)
    assert len(m) == 1, m
    out["SLAB_LDS_KB"] = int(m[0])
    m = re.findall(r'getenv\("SNK_WGRAD_NK"\)\s*\?\s*atoi\(getenv\("SNK_WGRAD_NK"\)\)\s*:\s*(\d+)\s*;', text)
    assert len(m) == 1, m
    out["NK_MAX"] = int(m[0])
    m = re.findall(r"height == width && \(width == (\d+) \|\| width == (\d+)\) \? width : 0;", text)
    assert len(m) == 1, m
    out["WT"] = (int(m[0][0]), int(m[0][1]))
    return out


def wg2_shape(h, w, c=None):
    """wg2_shape: (nk, maxx) of the window form, or None where it does not take the shape"""
    c = c or constants()
    if h < 1 or w < 3:
        return None
    P = w + 1
    nk = 5 if c["NK_MAX"] >= 5 else 4
    while nk >= 4:
        nxs = 16 * nk + 2 * P + 2
        rows_x = 16 * nk + c["WG_GX"] + 2 * P + 8
        lds = 2 * (4 * rows_x * 64 + 8 * 16 * nk * 64)
        maxx = (nxs * 16 + 511) // 512
        if maxx <= c["W2_MAXX"] and lds <= c["W2_LDS_KB"] * 1024:
            return nk, maxx
        nk -= 1
    return None


def wg_shape(h, w, c=None):
    """wg_shape: True where the slab form takes the shape"""
    c = c or constants()
    if h < 1 or w < 3:
        return False
    P = w + 1
    for n_slabs in range(1, h + 1):
        RB = (h + n_slabs - 1) // n_slabs
        nk = (RB * P + 15) // 16
        rows_x = 16 * nk + c["WG_GX"] + 2 * P + 8
        lds = 2 * 2 * 64 * (rows_x + 16 * nk)
        if (RB + 2) * w * 8 <= c["WG_MAXX"] * 256 and RB * w * 8 <= c["WG_MAXY"] * 256 and lds <= c["SLAB_LDS_KB"] * 1024:
            return True
    return False


def body(h, w, c=None):
    """the launch line of wgrad_launch at default settings (no SNK_WGRAD, no SNK_WGRAD_NK): (NK, MAXX, WT) or "slab"; ValueError where
    the launch is refused"""
    c = c or constants()
    s2 = wg2_shape(h, w, c)
    if s2 is None:
        if not wg_shape(h, w, c):
            raise ValueError(f"{h} x {w} images are not supported")
        return "slab"
    nk, maxx = s2
    wt = w if h == w and w in c["WT"] else 0
    if wt == 21 and nk == 5 and maxx <= 4:
        return (5, 4, 21)
    if wt == 21 and nk == 4 and maxx <= 4:
        return (4, 4, 21)
    if wt == 37 and nk == 4 and maxx <= 5:
        return (4, 5, 37)
    if nk == 5 and maxx <= 4:
        return (5, 4, 0)
    if nk == 5:
        return (5, 5, 0)
    if maxx <= 4:
        return (4, 4, 0)
    return (4, 5, 0)


def groups(n, h, w, slabs=False, c=None):
    """(groups, per_group, full, short, empty): the image groups of a launch, how many images a full one holds, how many groups are
    full, the image count of the one shorter group (0: there is none), how many groups hold no image.  slabs: under SNK_WGRAD=slabs"""
    c = c or constants()
    g = c["WG_GROUPS"] if slabs or body(h, w, c) == "slab" else c["WG2_GROUPS"]
    per = (n + g - 1) // g
    full, short = divmod(n, per)
    return g, per, full, short, g - full - (1 if short else 0)


# (n, H, W, body, (groups, per_group, full, short, empty)): what tests/test_wgrad_stream_gpu.py runs and why
CASES = [
    (129, 21, 21, (5, 4, 21), (128, 2, 64, 1, 63)),
    (300, 21, 21, (5, 4, 21), (128, 3, 100, 0, 28)),
    (130, 37, 37, (4, 5, 37), (128, 2, 65, 0, 63)),
    (385, 4, 13, (5, 4, 0), (128, 4, 96, 1, 31)),
    (513, 1, 3, (5, 4, 0), (128, 5, 102, 3, 25)),         # the smallest image: SR = 2
    (200, 6, 25, (5, 5, 0), (128, 2, 100, 0, 28)),
    (129, 5, 30, (4, 4, 0), (128, 2, 64, 1, 63)),
    (260, 3, 40, (4, 5, 0), (128, 3, 86, 2, 41)),
    (131, 21, 13, (5, 4, 0), (128, 2, 65, 1, 62)),        # H > W: the image pitch H + 1 above the row pitch W + 1
    (35, 3, 47, "slab", (16, 3, 11, 2, 4)),
]
# under SNK_WGRAD=slabs (a child process: the switch is read once): the two canvases of the BASELINE configs in the slab form
SLAB_SWITCH = [
    (33, 21, 21, (16, 3, 11, 0, 5)),
    (33, 37, 37, (16, 3, 11, 0, 5)),
]


def dw_ref(x, dy, dtype=None):
    """[3, 3, 128 ci, 128 co] from x, dy of [n, H, W, 128], on their device, in float64 (dtype: torch.float32 for the float32 yardstick)"""
    import torch
    dtype = dtype or torch.float64
    n, H, W, C = x.shape
    assert dy.shape == x.shape
    xp = torch.zeros(n, H + 2, W + 2, C, dtype=dtype, device=x.device)
    xp[:, 1:H + 1, 1:W + 1] = x
    g = dy.to(dtype).reshape(n * H * W, C)
    out = torch.empty(3, 3, C, C, dtype=dtype, device=x.device)
    for a in range(3):
        for b in range(3):
            out[a, b] = xp[:, a:a + H, b:b + W].reshape(n * H * W, C).t() @ g
    return out
