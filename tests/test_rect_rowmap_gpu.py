"""GPU tests of the packed sub-rectangle form's row map (csrc/conv_split.hip, hs_block<.., PK>: one table entry per GEMM row of
the block -- the output offset, -1 past the block's pixels, and the residual's source, the tensor or the producer's background
image -- written once per block into LDS and read by the epilogue).

The map changes where a row goes and where its shortcut comes from, never a value: the packed form has to give the full form's
bytes.  Hand-made bounding boxes put the cases a wrong entry would show in every launch: blocks of every tile count, blocks
whose second segment is another image or empty, rectangles on every canvas edge and corner (each of the four comparisons of
the "did the producer compute this pixel" test decides somewhere), a ring of `grow_res` rows on all four sides (both residual
sources inside one block and inside one 8-row group), on a 21 x 21 and on a 13 x 13 canvas.  Every activation tensor sits
between NaN guard regions: an entry of a row past the block's pixels must never be used as an address."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GUARD = 1 << 16          # floats in front of and behind every tensor
N_RECT = 6               # sub-rectangle layers on both canvases: three without a shortcut, three with one


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available()
    import snake_engine
    from snake_engine import net
    return torch, snake_engine, net


def _randomised_bn(ws, seed):
    rng = np.random.RandomState(seed)
    out = [w.copy() for w in ws]
    k = 0
    while k < len(out):
        if out[k].ndim == 4:
            n = out[k].shape[3]
            out[k + 1] = (1.0 + 0.2 * rng.randn(n)).astype(np.float32)
            out[k + 2] = (0.1 * rng.randn(n)).astype(np.float32)
            out[k + 3] = (0.05 * rng.randn(n)).astype(np.float32)
            out[k + 4] = (0.5 + rng.rand(n)).astype(np.float32)
            k += 5
        else:
            k += 1
    return out


def boxes_of(hw):
    """bounding boxes (y0, x0, y1, x1) on an hw x hw canvas, 8-40 of them.  Images of one rectangle shape share GEMM tiles, so
    every group below is several boxes of one size at different places:
      * the board window (hw = 2 board - 1) in the four corners, at the centre and off centre: from the second layer on
        their rectangles are (nearly) the whole canvas, the large blocks and the two-image blocks of 7-8 tiles
      * small squares in the four corners and at the middle of the four edges: the rectangle is clipped on one or two sides,
        so the ring of background residual rows is missing there and present on the others
      * small squares inside, far from every edge: the ring on all four sides; 1-4 tile blocks crossing image boundaries
      * two tall boxes and one shape nobody shares (a bin of one image: blocks with an empty second segment)"""
    b = (hw + 1) // 2
    far = hw - b
    out = [(0, 0, b - 1, b - 1), (0, far, b - 1, hw - 1), (far, 0, hw - 1, b - 1), (far, far, hw - 1, hw - 1),
           (far // 2, far // 2, far // 2 + b - 1, far // 2 + b - 1), (1, far - 2, b, hw - 3)]
    mid = hw // 2
    for s in (1, 2):
        out += [(0, 0, s - 1, s - 1), (0, hw - s, s - 1, hw - 1), (hw - s, 0, hw - 1, s - 1), (hw - s, hw - s, hw - 1, hw - 1),
                (0, mid, s - 1, mid + s - 1), (hw - s, mid, hw - 1, mid + s - 1), (mid, 0, mid + s - 1, s - 1),
                (mid, hw - s, mid + s - 1, hw - 1)]
    c = hw // 2 - 1
    for s, copies in ((1, 5), (2, 3), (3, 3)):
        out += [(c - k % 2, c + k % 3 - 1, c - k % 2 + s - 1, c + k % 3 - 1 + s - 1) for k in range(copies)]
    out += [(1, c, hw - 3, c + 1), (2, c - 1, hw - 2, c)]
    out.append((c, c - 1, c + 1, c + 3))
    assert 8 <= len(out) <= 40 and all(0 <= y0 <= y1 < hw and 0 <= x0 <= x1 < hw for y0, x0, y1, x1 in out)
    return out


def _boxed(torch, hw, box, seed):
    """an observation whose non-background pixels have exactly this bounding box"""
    y0, x0, y1, x1 = box
    g = torch.Generator().manual_seed(seed)
    t = torch.tensor([0.0, 1.0, 0.0]).repeat(hw, hw, 1)
    t[y0:y1 + 1, x0:x1 + 1] = torch.where(torch.rand(y1 - y0 + 1, x1 - x0 + 1, 1, generator=g) < 0.4,
                                          torch.rand(y1 - y0 + 1, x1 - x0 + 1, 3, generator=g), t[y0:y1 + 1, x0:x1 + 1])
    t[y0, x0] = torch.tensor([0.3, 0.2, 0.1]); t[y1, x1] = torch.tensor([0.7, 0.0, 0.4])
    return t


def _guarded(torch, shape):
    """a NaN-filled tensor of this shape with GUARD NaN floats in front of it and behind it, and the whole allocation"""
    n = int(np.prod(shape))
    whole = torch.full((n + 2 * GUARD,), float("nan"), device="cuda")
    return whole[GUARD:GUARD + n].view(shape), whole


@functools.lru_cache(maxsize=None)
def _towers(hw):
    """the stem and the sub-rectangle layers of one net on the hand-made observations, layer by layer, in the full form, the
    packed form and the unpacked form; computed once per canvas and shared by the tests (which do not change it)"""
    import os
    import torch
    import snake_engine  # noqa: F401
    from snake_engine import net
    from snake_engine._lib import check
    boxes = boxes_of(hw)
    planes = torch.stack([_boxed(torch, hw, b, 7 * i + hw) for i, b in enumerate(boxes)]).contiguous().cuda()
    m = planes.shape[0]
    ws = _randomised_bn(net.glorot_uniform_weights((hw, hw, 3), blocks=4, seed=hw), 5)
    keep = {k: os.environ.get(k) for k in ("SNK_CONV_RECT", "SNK_CONV_RECT_PACK", "SNK_CONV_RECT_LAYERS")}
    try:
        os.environ["SNK_CONV_RECT"] = "0"
        full = net.QNet(ws, (hw, hw, 3), max_chunk=8192)
        os.environ["SNK_CONV_RECT"] = "1"
        os.environ["SNK_CONV_RECT_LAYERS"] = str(N_RECT)     # (the 13 x 13 canvas takes three by default: too few for 8-tile shortcut blocks)
        os.environ["SNK_CONV_RECT_PACK"] = "1"
        pack = net.QNet(ws, (hw, hw, 3), max_chunk=8192)
        os.environ["SNK_CONV_RECT_PACK"] = "0"
        plain = net.QNet(ws, (hw, hw, 3), max_chunk=8192)
    finally:
        for k, v in keep.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    pack.rect_min = plain.rect_min = 1
    assert full.n_rect == 0 and pack.n_rect == N_RECT and pack.rect_pack and plain.n_rect == pack.n_rect and not plain.rect_pack
    st = torch.cuda.current_stream().cuda_stream

    def tower(qn, use_plan):
        made = [_guarded(torch, (m, hw, hw, 128)) for _ in range(3)]
        bufs, wholes = [a for a, _ in made], [w for _, w in made]
        check(qn.L.snk_stem_conv_bn_relu_f32(planes.data_ptr(), qn.stem_w.data_ptr(), qn.stem_sc.data_ptr(), qn.stem_sh.data_ptr(),
                                             bufs[0].data_ptr(), m, hw, hw, st))
        plan = qn._rect_plan(planes, m, 0, st) if use_plan else None
        outs, (cur, t1, t2) = [], bufs
        for i in range(pack.n_rect):
            if i % 2 == 0:
                qn._conv(i, cur, None, t1, m, st, plan=plan); outs.append(t1.clone())
            else:
                qn._conv(i, t1, cur, t2, m, st, plan=plan); outs.append(t2.clone())      # the shortcut path
                cur, t2 = t2, cur
        torch.cuda.synchronize()
        guards = [(w[:GUARD].clone(), w[-GUARD:].clone()) for w in wholes]
        return outs, plan, guards
    o_full, _, g_full = tower(full, False)
    o_pack, plan, g_pack = tower(pack, True)
    o_plain, plan_plain, g_plain = tower(plain, True)
    assert plan[4] and not plan_plain[4]                                 # the packed plan was taken, and the unpacked one
    n_rect = pack.n_rect
    desc = plan[0].cpu().numpy().view(np.uint32)
    counts = plan[1].cpu().numpy()
    blocks = [desc[i, :int(counts[i, 0])].reshape(-1, 8) for i in range(n_rect)]
    return dict(boxes=boxes, m=m, n_rect=n_rect, fill=list(pack.rect_fill[:n_rect]), full=o_full, pack=o_pack, plain=o_plain,
                blocks=blocks, guards=g_full + g_pack + g_plain)


def _valid(torch, t, i):
    """the pixels layer i's packed launch has to write: its rectangles, or every pixel where the layer fills the canvas"""
    hw = t["full"][0].shape[1]
    valid = torch.zeros((t["m"], hw, hw), dtype=torch.bool)
    for e in t["blocks"][i].reshape(-1, 4):
        fy, fx, fh, fw = e[1] & 255, (e[1] >> 8) & 255, (e[1] >> 16) & 255, e[1] >> 24
        valid[int(e[0]), fy:fy + fh, fx:fx + fw] = True
    return torch.ones_like(valid).cuda() if t["fill"][i] else valid.cuda()


@pytest.mark.parametrize("hw", [21, 13])
def test_the_hand_made_boxes_make_the_blocks_the_row_map_has_to_get_right(env, hw):
    """what the other tests rely on, read off the plan the device wrote: per epilogue mode (even layers: no shortcut, odd layers:
    shortcut) blocks of every tile count 1-8, blocks whose second segment is another image, blocks without one; rectangles on
    each canvas edge and in each corner, and rectangles with the background ring of the residual on all four sides"""
    torch, se, net = env
    t = _towers(hw)
    for mode, layers in ((1, range(0, t["n_rect"], 2)), (2, range(1, t["n_rect"], 2))):
        tiles, two, one = set(), 0, 0
        edges, ring4 = set(), 0
        for i in layers:
            d = t["blocks"][i]
            nB = d[:, 6] & 0xFFFF
            tiles |= set(((d[:, 6] >> 16) & 15).tolist())
            two += int(((nB > 0) & (d[:, 0] != d[:, 4])).sum())
            one += int((nB == 0).sum())
            for (y0, x0, y1, x1) in t["boxes"]:
                g, gr = i + 2, i                        # the layer's rectangle, and what the residual's producer computed
                top, left, bottom, right = y0 - g <= 0, x0 - g <= 0, y1 + g >= hw - 1, x1 + g >= hw - 1
                edges |= {k for k, on in zip("tlbr", (top, left, bottom, right)) if on}
                edges |= {a + b for a, b in ("tl", "tr", "bl", "br") if {"t": top, "l": left, "b": bottom, "r": right}[a]
                          and {"t": top, "l": left, "b": bottom, "r": right}[b]}
                ring4 += mode == 2 and y0 - gr > 0 and x0 - gr > 0 and y1 + gr < hw - 1 and x1 + gr < hw - 1
        print(f"{hw} x {hw}, MODE {mode}: tile counts {sorted(tiles)}, two-image blocks {two}, one-segment blocks {one}, "
              f"rectangles with the ring on four sides {ring4}")
        assert tiles >= set(range(1, 9)) and two > 0 and one > 0
        assert edges >= set("tlbr") | {"tl", "tr", "bl", "br"}
        assert mode == 1 or ring4 > 0


@pytest.mark.parametrize("hw", [21, 13])
def test_packed_and_unpacked_forms_give_the_full_form_bytes(env, hw):
    torch, se, net = env
    t = _towers(hw)
    assert t["n_rect"] >= 2                                              # both epilogue modes run
    for i in range(t["n_rect"]):
        v = _valid(torch, t, i)
        a = t["full"][i][v]
        assert torch.isfinite(a).all()
        assert torch.equal(a, t["pack"][i][v]), (i, "packed", (a - t["pack"][i][v]).abs().max().item())
        assert torch.equal(a, t["plain"][i][v]), (i, "unpacked", (a - t["plain"][i][v]).abs().max().item())
        if i < 2 and not t["fill"][i]:                                   # (first use of the NaN-filled buffer)
            assert torch.isnan(t["pack"][i][~v]).all()                   # nothing outside the rectangles is written


@pytest.mark.parametrize("hw", [21, 13])
def test_nothing_is_written_outside_the_tensors_and_nothing_read_there(env, hw):
    """NaN in front of and behind the input, the residual and the output of every launch: the guards keep their bits, and
    what the launches wrote is finite (a row past the block's pixels that was read or stored through its table entry, or a
    residual taken from outside its tensor, would show as one or the other)"""
    torch, se, net = env
    t = _towers(hw)
    for front, back in t["guards"]:
        assert torch.isnan(front).all() and torch.isnan(back).all()
        assert (front.view(torch.int32) == front.view(torch.int32)[0]).all() and (back.view(torch.int32) == front.view(torch.int32)[0]).all()
    for i in range(t["n_rect"]):
        v = _valid(torch, t, i)
        assert torch.isfinite(t["pack"][i][v]).all() and torch.isfinite(t["plain"][i][v]).all()
