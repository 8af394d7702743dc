"""GPU test of the packed sub-rectangle form (csrc/conv_split.hip: k_rect_plan_pack, k_conv3x3_f16s_rectp): the rectangles of
one shape share GEMM tiles, a block may hold the last rows of one image and the first rows of the next.  Which pixels share a
tile changes no accumulation order, so the outputs are the full form's bytes; and the plan the device writes is the one the host
build of the rule predicts for the same bounding boxes."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

H = W = 21


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


def _mid_game_planes(se, torch, n, board, snakes, ticks, seed):
    eng = se.Engine(n, board, board, snakes, 1, 0.15, seed=seed)
    eng.reset()
    g = torch.Generator(device="cuda").manual_seed(seed)
    for _ in range(ticks):
        pairs = torch.nonzero(eng.alive()).to(torch.int32).contiguous()
        _, mask, _ = eng.observe_all(pairs, want_planes=False, want_key=False)
        pick = torch.multinomial((mask == 0).to(torch.float32) + 1e-3, 1, generator=g).squeeze(1).to(torch.uint8)
        mv = torch.ones((n, snakes), dtype=torch.uint8, device="cuda")
        mv[pairs[:, 0].long(), pairs[:, 1].long()] = pick
        eng.step(mv)
    pairs = torch.nonzero(eng.alive()).to(torch.int32).contiguous()
    planes, _, _ = eng.observe_all(pairs)
    return planes


def _boxed(torch, y0, x0, y1, x1, seed):
    """an observation whose non-background pixels have exactly this bounding box"""
    g = torch.Generator().manual_seed(seed)
    t = torch.tensor([0.0, 1.0, 0.0]).repeat(H, W, 1)
    t[y0:y1 + 1, x0:x1 + 1] = torch.where(torch.rand(y1 - y0 + 1, x1 - x0 + 1, 1, generator=g) < 0.4,
                                          torch.rand(y1 - y0 + 1, x1 - x0 + 1, 3, generator=g), t[y0:y1 + 1, x0:x1 + 1])
    t[y0, x0] = torch.tensor([0.3, 0.2, 0.1]); t[y1, x1] = torch.tensor([0.7, 0.0, 0.4])
    return t


def _extras(torch):
    """small bins of hand-made shapes: a few images of one small shape make blocks that cross an image boundary at the small
    tile counts (a 5 x 5 rectangle is 25 pixels: a tile holds one and the head of the next), two 21 x 11 rectangles an 8-tile
    block of the end of one and the head of the other; and one shape nobody else has"""
    obs = []
    for s, copies in ((1, 5), (2, 5), (3, 5), (4, 3), (6, 5)):
        obs += [_boxed(torch, 10, 10, 10 + s - 1, 10 + s - 1, 10 * s + c) for c in range(copies)]
    obs += [_boxed(torch, 2, 5, 18, 11, 90 + c) for c in range(2)]
    obs.append(_boxed(torch, 9, 8, 11, 13, 99))                      # 3 x 6: a bin of one image in every layer
    return torch.stack(obs).contiguous()


def test_packed_form_gives_the_full_form_bytes_and_the_predicted_plan(env, monkeypatch):
    torch, se, net = env
    from snake_engine._lib import check
    ws = _randomised_bn(net.glorot_uniform_weights((H, W, 3), blocks=4, seed=11), 5)
    planes = torch.cat([_mid_game_planes(se, torch, 220, 11, 4, 12, seed=311), _extras(torch).cuda()]).contiguous()
    m = planes.shape[0]
    monkeypatch.setenv("SNK_CONV_RECT", "0")
    full = net.QNet(ws, (H, W, 3), max_chunk=8192)
    monkeypatch.setenv("SNK_CONV_RECT", "1")
    monkeypatch.setenv("SNK_CONV_RECT_PACK", "1")
    pack = net.QNet(ws, (H, W, 3), max_chunk=8192)
    pack.rect_min = 1
    assert full.n_rect == 0 and pack.n_rect == 6 and pack.rect_pack
    st = torch.cuda.current_stream().cuda_stream

    def tower(qn, use_plan):
        bufs = [torch.full((m, H, W, 128), float("nan"), device="cuda") for _ in range(3)]
        check(qn.L.snk_stem_conv_bn_relu_f32(planes.data_ptr(), qn.stem_w.data_ptr(), qn.stem_sc.data_ptr(), qn.stem_sh.data_ptr(),
                                             bufs[0].data_ptr(), m, H, W, st))
        plan = qn._rect_plan(planes, m, 0, st) if use_plan else None
        outs, (cur, t1, t2) = [], bufs
        for i in range(6):
            if i % 2 == 0:
                qn._conv(i, cur, None, t1, m, st, plan=plan); outs.append(t1.clone())
            else:
                qn._conv(i, t1, cur, t2, m, st, plan=plan); outs.append(t2.clone())      # the shortcut path
                cur, t2 = t2, cur
        return outs, plan
    o_full, _ = tower(full, False)
    o_pack, plan = tower(pack, True)
    assert plan[4]                                                       # the packed plan was taken
    torch.cuda.synchronize()
    desc = plan[0].cpu().numpy().view(np.uint32)
    counts = plan[1].cpu().numpy()
    bbox = plan[3][:m].cpu().numpy().view(np.uint32)
    L = pack.L
    crossing, lone_bin = set(), False
    for i in range(6):
        nd = int(counts[i, 0])
        d = desc[i, :nd].reshape(-1, 8)
        # the device's plan against the host build of the rule on the same bounding boxes
        md = L.snk_conv_rect_pack_max_desc(m, H, W)
        assert md == desc.shape[1]
        hd = np.zeros((md, 4), dtype=np.uint32)
        hc = np.zeros(2, dtype=np.int32)
        assert L.snk_conv_rect_plan_pack_host(bbox.ctypes.data_as(C.c_void_p), m, H, W, i + 2, hd.ctypes.data_as(C.c_void_p),
                                              hc.ctypes.data_as(C.c_void_p)) == 0
        print(f"layer {i}: device entries {nd} tiles {int(counts[i, 1])}; host entries {int(hc[0])} tiles {int(hc[1])}")
        assert (nd, int(counts[i, 1])) == (int(hc[0]), int(hc[1]))
        h8 = hd[:hc[0]].reshape(-1, 8)
        key = lambda a: sorted(zip((a[:, 1] >> 16).tolist(), a[:, 2].tolist(), a[:, 6].tolist()))     # (shape, cut) of every block
        assert key(d) == key(h8)
        nt = (d[:, 6] >> 16) & 15
        assert (nt[:-1] >= nt[1:]).all()                                 # largest first
        crossing |= set(nt[(d[:, 6] & 0xFFFF) > 0].tolist())
        per_shape = {}
        for img, rc in set(zip(d[:, 0].tolist(), (d[:, 1] >> 16).tolist())) | set(zip(d[:, 4].tolist(), (d[:, 5] >> 16).tolist())):
            per_shape[rc] = per_shape.get(rc, 0) + 1
        assert sum(per_shape.values()) == m                              # every image, once
        lone_bin |= 1 in per_shape.values()
        # bytes: on the rectangles, and on the whole canvas where the layer fills
        valid = torch.zeros((m, H, W), dtype=torch.bool)
        for e in desc[i, :nd]:
            fy, fx, fh, fw = e[1] & 255, (e[1] >> 8) & 255, (e[1] >> 16) & 255, e[1] >> 24
            valid[int(e[0]), fy:fy + fh, fx:fx + fw] = True
        v = valid.cuda()
        if pack.rect_fill[i]:
            v = torch.ones_like(v)
        elif i < 2:
            assert torch.isnan(o_pack[i][~v]).all()                      # nothing outside the rectangles is written
        a, b = o_full[i][v], o_pack[i][v]
        assert torch.isfinite(a).all()
        assert torch.equal(a, b), (i, (a - b).abs().max().item())
    assert pack.rect_fill[5]
    print("tile counts of blocks that cross an image boundary:", sorted(crossing))
    assert crossing >= set(range(1, 9)) and lone_bin
    # and the whole net, in one chunk and in ragged ones
    q_full = full.forward(planes)
    assert torch.isfinite(q_full).all() and torch.equal(pack.forward(planes), q_full)
    pack.max_chunk = 53
    assert torch.equal(pack.forward(planes), q_full)
    # the unpacked plan stays selectable and gives the same bytes
    monkeypatch.setenv("SNK_CONV_RECT_PACK", "0")
    plain = net.QNet(ws, (H, W, 3), max_chunk=8192)
    plain.rect_min = 1
    assert not plain.rect_pack and torch.equal(plain.forward(planes), q_full)
