"""tests/rect16_ref.py on its own: the constants are found, parts() is the smallest feasible cut, the case list of
tests/test_rect16_gpu.py covers the kernel bodies and edges it is meant to, and the one-hot model tells the faults apart that the
GPU test exists to catch.  No GPU, no library."""
import numpy as np
import pytest

import conv_plan_ref as cp
import rect16_ref as rr


def test_the_constants_are_found_in_the_source():
    c = rr.constants()
    assert set(c) == {"HS_NST16", "HS_BUF16", "HS_LDP", "HS_GAP16_RECT"}
    assert all(v > 0 for v in c.values())
    both = cp.constants()
    assert all(c[k] == both[k] for k in ("HS_NST16", "HS_BUF16", "HS_LDP"))      # the same #defines, read twice


def _smallest_feasible(hr, wr, H, W, c):
    """the fewest parts of at most 8 tiles whose strip fits, found by trying every count and every alignment of a part"""
    T = -(-hr * wr // 32)
    for n in range(1, T + 1):
        tm = -(-T // n)
        if tm > 8:
            continue
        rows = min(max((off + 32 * tm - 1) // wr + 1 for off in range(wr)), hr)      # rows a run of 32 tm pixels touches
        lds_bytes = (rows + 2) * ((wr + 2) * c["HS_LDP"] + c["HS_GAP16_RECT"])       # + one row above, one below, two halo columns
        staged = min(rows + 2, H) * min(wr + 2, W)                                   # the strip's pixels on the canvas
        if lds_bytes <= c["HS_BUF16"] and staged <= 64 * c["HS_NST16"]:
            return n, tm
    return -1, 1


@pytest.mark.parametrize("H,W", [(37, 37), (9, 13)])
def test_parts_is_the_smallest_feasible_count_for_every_shape(H, W):
    c = rr.constants()
    for hr in range(1, H + 1):
        for wr in range(1, W + 1):
            p = rr.parts(hr, wr, H, W, c)
            assert (p.parts, p.tiles_max) == _smallest_feasible(hr, wr, H, W, c), (hr, wr)
            T = -(-hr * wr // 32)
            assert (p.lds or p.staging) == (p.parts > -(-T // 8)), (hr, wr)
            tiles = rr.part_tiles(hr, wr, H, W, c)
            assert [t for t, _ in tiles] == [sum(n for _, n in tiles[:k]) for k in range(len(tiles))]
            assert sum(n for _, n in tiles) == T and max(n for _, n in tiles) == p.tiles_max and min(n for _, n in tiles) >= 1
    assert rr.max_blocks(3, H, W, c) == 3 * max(rr.parts(a, b, H, W, c).parts for a in range(1, H + 1) for b in range(1, W + 1))


def _f32_parts(hr, wr, H, W, c):
    """hs_rect_parts of the float32 frame (tests/test_rect_conv_gpu.py::_parts, with the constants read from the source)"""
    T = -(-hr * wr // 32)
    n = -(-T // 8)
    while True:
        tm = -(-T // n)
        rows = min((tm * 32 + wr - 2) // wr + 1, hr)
        if (rows + 2) * (wr + 2) <= c["HS_NPB"] and min(rows + 2, H) * min(wr + 2, W) <= 64 * c["HS_NST"]:
            return n, tm
        assert tm > 1
        n += 1


def test_the_16_bit_plan_is_not_the_float32_plan_on_37x37():
    """with today's constants: 437 of the 1369 shapes are cut differently, and 72 need more parts than ceil(T / 8)"""
    c, c32 = rr.constants(), cp.constants()
    shapes = [(hr, wr) for hr in range(1, 38) for wr in range(1, 38)]
    differ = sum(tuple(rr.parts(hr, wr, 37, 37, c)[:2]) != _f32_parts(hr, wr, 37, 37, c32) for hr, wr in shapes)
    limited = sum(rr.parts(hr, wr, 37, 37, c).parts > -(-(-(-hr * wr // 32)) // 8) for hr, wr in shapes)
    assert differ > 0 and limited > 0
    assert (differ, limited) == (437, 72), "a frame constant changed: look at the case list's coverage below"


def _shapes_37():
    return [(g, box, rr.rect_of(box, g, 37, 37)) for g in rr.GROW for box in rr.CASES_37]


def test_the_case_list_covers_what_it_is_meant_to():
    """if a frame constant changes so that this fails, the list is changed, not the assertion"""
    c = rr.constants()
    shapes = _shapes_37()
    ps = [rr.parts(hr, wr, 37, 37, c) for _, _, (_, _, hr, wr) in shapes]
    ntiles = {n for _, _, (_, _, hr, wr) in shapes for _, n in rr.part_tiles(hr, wr, 37, 37, c)}
    assert ntiles == set(range(1, 9))
    counts = {p.parts for p in ps}
    assert {1, 2, rr.parts(37, 37, 37, 37, c).parts} <= counts and any(n >= 3 for n in counts)
    assert any(p.lds for p in ps) and any(p.staging and not p.lds for p in ps)
    edges = [(y0 == 0, x0 == 0, y0 + hr == 37, x0 + wr == 37) for _, _, (y0, x0, hr, wr) in shapes]
    assert all(any(e[k] for e in edges) for k in range(4)) and any(not any(e) for e in edges)
    assert any(hr * wr % 32 == 0 for _, _, (_, _, hr, wr) in shapes) and any(hr * wr % 32 for _, _, (_, _, hr, wr) in shapes)
    assert any(wr == 1 for _, _, (_, _, hr, wr) in shapes) and any(hr == 1 for _, _, (_, _, hr, wr) in shapes)


def test_grow_one_alone_reaches_every_tile_count():
    """what the issue that asked for these tests states of today's constants: rectangle grow 1 runs ntile 1 .. 8, part counts 1, 2, 3
    and 6, the shape 13 x 35 that both constraints cut to [5, 5, 5] and the shape 14 x 33 that only the staging items limit"""
    c = rr.constants()
    shapes = [rr.rect_of(box, 1, 37, 37)[2:] for box in rr.CASES_37]
    assert {n for hr, wr in shapes for _, n in rr.part_tiles(hr, wr, 37, 37, c)} == set(range(1, 9))
    assert {rr.parts(hr, wr, 37, 37, c).parts for hr, wr in shapes} >= {1, 2, 3, 6}
    assert (13, 35) in shapes and rr.parts(13, 35, 37, 37, c) == rr.Parts(3, 5, True, True)
    assert [n for _, n in rr.part_tiles(13, 35, 37, 37, c)] == [5, 5, 5]
    assert (14, 33) in shapes and rr.parts(14, 33, 37, 37, c)[2:] == (False, True)


def test_the_plan_model_covers_every_tile_once_and_bins_by_the_largest_part():
    c = rr.constants()
    for H, W, boxes in rr.CANVASES:
        for g, lp in zip(rr.GROW, rr.plan(boxes, rr.GROW, H, W, c)):
            assert [tm for tm, _ in lp.bins] == sorted((tm for tm, _ in lp.bins), reverse=True)
            seen = {}
            for tm, descs in lp.bins:
                for img, rect, tl, bw in descs:
                    assert bw == rr.box_word(boxes[img]) and (tl >> 8) & 255 <= tm
                    seen.setdefault(img, []).append((tl & 255, (tl >> 8) & 255, (tl >> 16) & 255, tl >> 24, rect, tm))
            assert sorted(seen) == list(range(len(boxes)))
            for img, ds in seen.items():
                y0, x0, hr, wr = rr.rect_of(boxes[img], g, H, W)
                nxt = 0
                for k, (t0, nt, part, n, rect, tm) in enumerate(sorted(ds)):
                    assert (t0, part, n, rect) == (nxt, k, len(ds), y0 | x0 << 8 | hr << 16 | wr << 24)
                    nxt += nt
                assert nxt == -(-hr * wr // 32) and max(d[1] for d in ds) == ds[0][5]
            assert lp.count == sum(len(d) for d in seen.values()) <= rr.max_blocks(len(boxes), H, W, c)
            assert lp.tiles == sum(-(-np.prod(rr.rect_of(b, g, H, W)[2:]) // 32) for b in boxes)


def test_compose_and_layer_on_a_small_example():
    """compose keeps x on the grown, cut box; layer() of a one-hot kernel equals one_hot_expected(); zero padding at the canvas edge"""
    rng = np.random.RandomState(0)
    H, W, C = 5, 6, 4
    boxes = [(0, 0, 1, 1), (2, 3, 2, 3)]
    x, bg = rng.randn(2, H, W, C), rng.randn(H, W, C)
    r, bgr = rng.randn(2, H, W, C), rng.randn(H, W, C)
    xc = rr.compose(x, bg, boxes, 1, H, W)
    assert np.array_equal(xc[0, :3, :3], x[0, :3, :3]) and np.array_equal(xc[0, 3:], bg[3:]) and np.array_equal(xc[0, :, 3:], bg[:, 3:])
    assert np.array_equal(xc[1, 1:4, 2:5], x[1, 1:4, 2:5]) and np.array_equal(xc[1, 0], bg[0]) and np.array_equal(xc[1, :, 5], bg[:, 5])
    assert np.array_equal(rr.compose(x[1], bg, boxes[1], 1, H, W), xc[1])
    for tap in range(9):
        w = np.zeros((3, 3, C, C))
        w[tap // 3, tap % 3] = np.eye(C)
        got = rr.layer(x, bg, boxes, 1, w, np.ones(C), np.zeros(C), r, bgr, 0)
        assert np.array_equal(got, rr.one_hot_expected(x, bg, boxes, 1, tap, r, bgr, 0))
    w = np.zeros((3, 3, C, C))
    w[0, 0] = np.eye(C)                                       # tap 0 reads (y - 1, x - 1): row 0 and column 0 see the zero border
    out = rr.layer(x, bg, boxes, 1, w, np.ones(C), np.zeros(C))
    assert not out[:, 0].any() and not out[:, :, 0].any() and np.array_equal(out[:, 1:, 1:], np.maximum(xc[:, :-1, :-1], 0))


def _one_hot_data(H, W, boxes, seed):
    """integers |v| <= 15 times 2^-2 .. 2^2 per 32-channel block (exact in f16, bf16 and MX-FP8), as the GPU test's"""
    rng = np.random.RandomState(seed)
    n = len(boxes)

    def t(*lead):
        return rng.randint(-15, 16, size=lead + (128,)) * np.repeat(np.exp2(rng.randint(-2, 3, size=lead + (4,))), 32, axis=-1)
    return t(n, H, W), t(H, W), t(n, H, W), t(H, W)


MUTANTS = {
    "grow_in + 1": dict(d_in=1),
    "grow_in - 1": dict(d_in=-1),
    "zero border -> background": dict(border="bg"),
    "stale pixels from x": dict(stale="x"),
    "grow_res + 1": dict(d_res=1),
    "grow_res - 1": dict(d_res=-1),
}


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_the_one_hot_model_tells_each_fault_apart(mutant):
    """over the case list and the production grows, the expected output ON THE RECTANGLES differs from the mutant's for at least
    one tap and element: a kernel with that fault fails tests/test_rect16_gpu.py"""
    m = MUTANTS[mutant]
    H = W = 37
    boxes = rr.CASES_37
    x, bg, r, bgr = _one_hot_data(H, W, boxes, 5)
    with_res = "d_res" in m or "stale" in m
    differs = 0
    for g in rr.GROW:
        gi, gr = max(g - 1, 0), max(g - 2, 0)
        on = rr.inside(boxes, g, H, W)[..., None]
        for tap in range(9):
            res = (r, bgr, gr) if with_res else (None, None, 0)
            want = rr.one_hot_expected(x, bg, boxes, gi, tap, *res)
            got = rr.one_hot_expected(x, bg, boxes, gi + m.get("d_in", 0), tap, res[0], res[1], gr + m.get("d_res", 0),
                                      border=m.get("border", "zero"), stale=m.get("stale", "bg"))
            differs += int(((want != got) & on).sum())
    assert differs > 0
