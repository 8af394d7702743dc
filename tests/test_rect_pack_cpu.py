"""The packed plan of the float32-accurate sub-rectangle layers (csrc/conv_split.hip: hs_pack_walk, k_rect_plan_pack), driven
through the library's host build of the rule (snk_conv_rect_plan_pack_host) -- no GPU.

Every rectangle alone pads its pixels to whole 32-row GEMM tiles; the packed plan gives the rectangles of one shape a shared
row space.  Checked here: every pixel of every rectangle is covered exactly once, no block exceeds 8 tiles, two segments, the
LDS pixel budget or the staging budget, and the plan executes fewer tiles than the unpacked rule -- at least 4 % fewer over
tower layers 0-5 on the benchmark's geometry (11 x 11 board on a 21 x 21 canvas, heads uniform over the board; the ideal,
no padding at all, is 5.2 %)."""
import ctypes as C

import numpy as np
import pytest

NPB_PACK = 416        # HS_NPB_PK: LDS pixels per staging buffer of the packed form (2 x 416 x 80 bytes <= the epilogue's 67 584)
NST_PIXELS = 320      # 64 x HS_NST canvas pixels a block stages per chunk
NPB, H, W = 352, 21, 21


@pytest.fixture(scope="module")
def L():
    import snake_engine
    return snake_engine.lib()


def _box(y0, x0, y1, x1):
    return y0 | x0 << 8 | y1 << 16 | x1 << 24


def _rect(b, g, h, w):
    y0, x0 = max((b & 255) - g, 0), max(((b >> 8) & 255) - g, 0)
    y1, x1 = min(((b >> 16) & 255) + g, h - 1), min((b >> 24) + g, w - 1)
    return y0, x0, y1 - y0 + 1, x1 - x0 + 1


def _old_parts(hr, wr, h, w):
    """the unpacked rule (hs_rect_parts): the fewest equal parts of at most 8 tiles whose strip fits 352 LDS pixels and 320
    staged pixels"""
    T = (hr * wr + 31) // 32
    parts = (T + 7) // 8
    while True:
        tm = (T + parts - 1) // parts
        rows_out = min((tm * 32 + wr - 2) // wr + 1, hr)
        if (rows_out + 2) * (wr + 2) <= NPB and min(rows_out + 2, h) * min(wr + 2, w) <= NST_PIXELS:
            return parts
        assert tm > 1
        parts += 1


def _old_blocks(hr, wr, h, w):
    T, parts = (hr * wr + 31) // 32, _old_parts(hr, wr, h, w)
    base, rem = divmod(T, parts)
    out = []
    for k in range(parts):
        t0, nt = k * base + min(k, rem), base + (1 if k < rem else 0)
        out.append((32 * t0, min(32 * (t0 + nt), hr * wr) - 32 * t0, nt))
    return out


def _plan(L, boxes, h, w, grow):
    n = len(boxes)
    md = L.snk_conv_rect_pack_max_desc(n, h, w)
    assert md > 0 and md % 2 == 0
    bb = np.asarray(boxes, dtype=np.uint32)
    desc = np.full((md, 4), 0xFFFFFFFF, dtype=np.uint32)
    counts = np.zeros(2, dtype=np.int32)
    rc = L.snk_conv_rect_plan_pack_host(bb.ctypes.data_as(C.c_void_p), n, h, w, grow, desc.ctypes.data_as(C.c_void_p),
                                        counts.ctypes.data_as(C.c_void_p))
    assert rc == 0, L.snk_last_error()
    assert counts[0] % 2 == 0 and counts[0] <= md and (desc[counts[0]:] == 0xFFFFFFFF).all()
    return desc[:counts[0]].reshape(-1, 8), int(counts[1])


def _strip(y_first, y_last, ry, rx, wr, h, w):
    """(LDS rows, staged canvas pixels) of a segment whose pixels span rectangle rows y_first .. y_last"""
    ya, yb = max(ry + y_first - 1, 0), min(ry + y_last + 1, h - 1)
    xa, xb = max(rx - 1, 0), min(rx + wr, w - 1)
    return y_last - y_first + 3, (yb - ya + 1) * (xb - xa + 1)


def _check(blocks, tiles, boxes, h, w, grow):
    """the invariants of a plan; returns the blocks per image as {image: [(first pixel, pixels)]}"""
    n = len(boxes)
    rects = [_rect(b, grow, h, w) for b in boxes]
    cover = [np.zeros(r[2] * r[3], dtype=np.int32) for r in rects]
    per_image = {}
    nts = []
    for ia, ra, za, ba, ib, rb, zb, bbx in blocks.tolist():
        m, nA, nB, nt = za & 0xFFFF, za >> 16, zb & 0xFFFF, (zb >> 16) & 15
        assert ia < n and ib < n
        ry, rx, hr, wr = rects[ia]
        S = hr * wr
        assert ra == ry | rx << 8 | hr << 16 | wr << 24 and ba == boxes[ia]
        ryb, rxb, hrb, wrb = rects[ib]
        assert rb == ryb | rxb << 8 | hrb << 16 | wrb << 24 and bbx == boxes[ib] and (hrb, wrb) == (hr, wr)
        assert nA >= 1 and m + nA <= S and 0 <= nB <= S
        assert nt == (nA + nB + 31) // 32 and 1 <= nt <= 8               # at most 8 tiles, at most two segments by construction
        if nB:
            assert ib != ia and m + nA == S                                # the second segment continues where an image ended
        else:
            assert ib == ia                                                # every 16-byte entry names an image and its rectangle
        cover[ia][m:m + nA] += 1
        per_image.setdefault(ia, []).append((m, nA))
        rows, staged = _strip(m // wr, (m + nA - 1) // wr, ry, rx, wr, h, w)
        if nB:
            cover[ib][:nB] += 1
            per_image.setdefault(ib, []).append((0, nB))
            r2, s2 = _strip(0, (nB - 1) // wr, ryb, rxb, wr, h, w)
            rows, staged = rows + r2, staged + s2
        assert rows * (wr + 2) <= NPB_PACK and staged <= NST_PIXELS, (hr, wr, m, nA, nB)
        nts.append(nt)
    assert all((c == 1).all() for c in cover)                              # every pixel of every rectangle exactly once
    assert nts == sorted(nts, reverse=True)                                # largest blocks first
    assert sum(nts) == tiles
    return per_image


def _bench_boxes(n):
    """the 121 head positions of an 11 x 11 board: the board window on the 21 x 21 canvas with the observer's head at its centre"""
    pos = [(10 - hy, 10 - hx) for hy in range(11) for hx in range(11)]
    return [_box(y, x, y + 10, x + 10) for y, x in (pos[i % 121] for i in range(n))]


def test_packed_plan_on_the_benchmark_geometry(L):
    boxes = _bench_boxes(8192)
    old_total = new_total = 0
    for layer in range(6):
        grow = layer + 2
        blocks, tiles = _plan(L, boxes, H, W, grow)
        _check(blocks, tiles, boxes, H, W, grow)
        old = sum((r[2] * r[3] + 31) // 32 for r in (_rect(b, grow, H, W) for b in boxes))
        ideal = sum(r[2] * r[3] for r in (_rect(b, grow, H, W) for b in boxes)) / 32.0
        print(f"layer {layer}: tiles {tiles} (unpacked {old}, pixels / 32 = {ideal:.0f}), blocks {len(blocks)}")
        assert tiles <= old
        old_total += old
        new_total += tiles
    print(f"layers 0-5: {new_total} tiles against {old_total}: {100.0 * (1 - new_total / old_total):.2f} % fewer")
    assert new_total <= 0.96 * old_total


def test_mixed_shapes(L):
    rng = np.random.RandomState(3)
    for h, w in ((21, 21), (37, 37), (21, 13)):
        boxes = []
        for _ in range(100):
            y0, y1 = sorted(rng.randint(0, h, 2)); x0, x1 = sorted(rng.randint(0, w, 2))
            boxes.append(_box(int(y0), int(x0), int(y1), int(x1)))
        boxes += boxes[:7] * 5                         # a few bins with several images
        for grow in (0, 2, 5):
            blocks, tiles = _plan(L, boxes, h, w, grow)
            _check(blocks, tiles, boxes, h, w, grow)
            assert tiles <= sum((r[2] * r[3] + 31) // 32 for r in (_rect(b, grow, h, w) for b in boxes))


def test_nothing_to_pack_degrades_to_the_unpacked_blocks(L):
    """every image has its own shape: each bin holds one image, and the plan is the unpacked rule's blocks"""
    boxes = [_box(5, 5, 5 + a, 5 + b) for a in range(11) for b in range(11)]
    grow = 2
    blocks, tiles = _plan(L, boxes, H, W, grow)
    per_image = _check(blocks, tiles, boxes, H, W, grow)
    assert (blocks[:, 6] & 0xFFFF == 0).all()          # no second segment anywhere
    assert len({_rect(b, grow, H, W)[2:] for b in boxes}) == len(boxes)
    for i, b in enumerate(boxes):
        _, _, hr, wr = _rect(b, grow, H, W)
        assert sorted(per_image[i]) == [(m, rows) for m, rows, _ in _old_blocks(hr, wr, H, W)]
    assert tiles == sum((r[2] * r[3] + 31) // 32 for r in (_rect(b, grow, H, W) for b in boxes))


def test_entry_points_refuse_bad_arguments(L):
    assert L.snk_conv_rect_pack_max_desc(4, 2, 21) < 0 and L.snk_conv_rect_pack_max_desc(4, 80, 80) < 0
    assert L.snk_conv_rect_pack_max_desc(0, 21, 21) >= 0
    c = np.zeros(2, dtype=np.int32)
    assert L.snk_conv_rect_plan_pack_host(None, 1, 21, 21, 2, None, c.ctypes.data_as(C.c_void_p)) < 0
