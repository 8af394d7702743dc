"""GPU tests of the MX-FP8 tower (SNK_CONV_ALGO=mxfp8, csrc/conv_split.hip hs_block<MX>): the staging quantizer byte for byte
against the rule's restatement (tests/mxfp8_ref.py), the MFMA's lane maps through a layer on exact integer data, a random layer
against a float64 convolution of the quantized operands, the sub-rectangle form against the full form, the whole net against
the restatement with the same rounding points and against the float32 net, one root turn of the search, and the entry points'
refusals of bad arguments.  Sizes are small: a few hundred images at most."""
import os

import numpy as np
import pytest

import mxfp8_ref as mx
from conftest import load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available()
    import snake_engine
    from snake_engine import net
    from snake_engine._lib import lib
    return torch, snake_engine, net, lib()


def _st():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _randomised_bn(ws, seed):
    """Glorot kernels with random batch-norm parameters (as tests/test_net_gpu.py)"""
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


def _bf16_edge_blocks():
    """hand-picked blocks (bf16-exact values): zeros, amax = 448 2^k, just above a power of two and above 1.75 2^k,
    subnormal codes, ties to even, an exponent that clamps at -127"""
    rows = [[0.0], [448.0, -448.0, 1.0], [448.0 * 2.0 ** 5, 3.0], [448.0 * 2.0 ** -20, -1.0 * 2.0 ** -20],
            [1.0078125, 0.5], [451.5, 3.0], [448.0, 2.0 ** -9, 3 * 2.0 ** -10, 2.0 ** -10, 0.75 * 2.0 ** -9, 7 * 2.0 ** -9, 2.0 ** -6],
            [448.0, 1.0625, 1.1875, -1.0625, 248.0, 216.0], [2.0 ** -130, -(2.0 ** -131), 2.0 ** -133]]
    out = np.zeros((len(rows), 32), np.float32)
    for i, r in enumerate(rows):
        out[i, :len(r)] = r
    return out


def test_quantizer_matches_the_rule_byte_for_byte(env):
    torch, _, _, L = env
    from snake_engine._lib import check
    rng = np.random.RandomState(1)
    n = 8192
    # magnitudes over about 2^-40 .. 2^40 per block, and spread inside a block (down into e4m3's subnormals and to zero)
    x = rng.randn(n, 32) * np.exp2(rng.randint(-40, 41, size=(n, 1))) * np.exp2(-rng.randint(0, 14, size=(n, 32)))
    x[rng.rand(n, 32) < 0.05] = 0.0
    x = np.concatenate([x.astype(np.float32), _bf16_edge_blocks()])
    xb = torch.as_tensor(x).to(torch.bfloat16)
    xf = xb.float().numpy()                                   # the bf16 values, exact in float32
    nb = xf.shape[0]
    codes = torch.full((nb, 32), 0x7F, dtype=torch.uint8, device="cuda")
    scales = torch.full((nb,), 255, dtype=torch.uint8, device="cuda")
    check(L.snk_mxfp8_quantize_bf16(xb.cuda().data_ptr(), nb, codes.data_ptr(), scales.data_ptr(), _st()))
    want_c, want_s = mx.quantize_blocks(xf)
    got_c, got_s = codes.cpu().numpy(), scales.cpu().numpy()
    assert np.array_equal(got_s, want_s), np.flatnonzero(got_s != want_s)[:8]
    bad = ~(((got_c == want_c) | (((got_c & 0x7F) == 0) & ((want_c & 0x7F) == 0))))
    assert not bad.any(), (np.argwhere(bad)[:8], got_c[bad][:8], want_c[bad][:8])
    assert mx.same_codes(got_c, want_c)


def _conv64(x, w):
    """float64 cross-correlation, 'same' padding: x [n][h][w][128], w [3][3][128][128] (HWIO) -> [n][h][w][128]"""
    import torch
    t = torch.nn.functional.conv2d(torch.as_tensor(x, dtype=torch.float64).permute(0, 3, 1, 2),
                                   torch.as_tensor(w, dtype=torch.float64).permute(3, 2, 0, 1), padding=1)
    return t.permute(0, 2, 3, 1).numpy()


@pytest.mark.parametrize("hw", [21, 37])
def test_exact_integer_layer_lane_maps(env, hw):
    """Inputs and weights are small integers (|v| <= 15) times a power of two (2^-2 .. 2^2) that varies per 32-channel block:
    their MX codes are exact, every product and partial sum is exact in float32, so the float32-output layer equals the float64
    convolution EXACTLY -- a wrong A, B or scale lane map of v_mfma_scale_f32_32x32x64_f8f6f4 shows as a difference.  Weights
    are random (asymmetric).  n = 1 / 40 cut images into one-tile blocks (the small-batch path), 300 runs the normal frame."""
    torch, _, net, L = env
    from snake_engine._lib import check
    rng = np.random.RandomState(hw)
    w = (rng.randint(-15, 16, size=(3, 3, 128, 128)) *
         np.repeat(np.exp2(rng.randint(-2, 3, size=(3, 3, 4, 128))), 32, axis=2)).astype(np.float32)
    wS = torch.empty(net.F16S_WEIGHT_BYTES, dtype=torch.uint8, device="cuda")
    check(L.snk_conv3x3_prepare_weights_mxfp8(torch.as_tensor(w).cuda().data_ptr(), wS.data_ptr(), _st()))
    one, zero = torch.ones(128, device="cuda"), torch.zeros(128, device="cuda")
    for n in (1, 40, 300):
        x = (rng.randint(-15, 16, size=(n, hw, hw, 128)) *
             np.repeat(np.exp2(rng.randint(-2, 3, size=(n, hw, hw, 4))), 32, axis=3)).astype(np.float32)
        r = (rng.randint(-15, 16, size=(n, hw, hw, 128)) * 0.25).astype(np.float32)
        xd = torch.as_tensor(x).to(torch.bfloat16).cuda()
        rd = torch.as_tensor(r).to(torch.bfloat16).cuda()
        pick = sorted({0, n // 2, n - 1, min(7, n - 1), min(8, n - 1)})
        ref = _conv64(x[pick], w)
        for res in (False, True):
            o = torch.full((n, hw, hw, 128), float("nan"), device="cuda")
            check(L.snk_conv3x3_bn_mxfp8_act16(xd.data_ptr(), wS.data_ptr(), one.data_ptr(), zero.data_ptr(),
                                               rd.data_ptr() if res else None, o.data_ptr(), 0, n, hw, hw, int(res), _st()))
            got = o.cpu().numpy()[pick].astype(np.float64)
            want = np.maximum(ref + r[pick], 0.0) if res else ref
            assert np.array_equal(got, want), (n, res, np.abs(got - want).max(), np.argwhere(got != want)[:4])


def test_random_layer_against_the_dequantized_operands(env):
    """random bf16 inputs, Glorot weights: the float32 output matches a float64 convolution of the restatement's dequantized
    operands within 2e-5 max|ref|; the bf16 output is that result rounded once"""
    torch, _, net, L = env
    from snake_engine._lib import check
    g = np.random.RandomState(11)
    lim = np.sqrt(6.0 / (2 * 9 * 128))
    for n, hw in ((3, 21), (2, 37)):
        x = torch.as_tensor(g.randn(n, hw, hw, 128).astype(np.float32)).to(torch.bfloat16)
        r = torch.as_tensor(g.randn(n, hw, hw, 128).astype(np.float32)).to(torch.bfloat16)
        w = g.uniform(-lim, lim, size=(3, 3, 128, 128)).astype(np.float32)
        sc, sh = (g.rand(128) + 0.5).astype(np.float32), (g.randn(128) * 0.1).astype(np.float32)
        ref = _conv64(mx.mx_round(x.float().numpy(), axis=3), mx.mx_round(w, axis=2))
        ref = np.maximum(ref * sc + sh + r.double().numpy(), 0.0)
        wS = torch.empty(net.F16S_WEIGHT_BYTES, dtype=torch.uint8, device="cuda")
        check(L.snk_conv3x3_prepare_weights_mxfp8(torch.as_tensor(w).cuda().data_ptr(), wS.data_ptr(), _st()))
        xd, rd, scd, shd = x.cuda(), r.cuda(), torch.as_tensor(sc).cuda(), torch.as_tensor(sh).cuda()
        o32 = torch.full((n, hw, hw, 128), float("nan"), device="cuda")
        check(L.snk_conv3x3_bn_mxfp8_act16(xd.data_ptr(), wS.data_ptr(), scd.data_ptr(), shd.data_ptr(), rd.data_ptr(),
                                           o32.data_ptr(), 0, n, hw, hw, 1, _st()))
        scale = np.abs(ref).max()
        assert np.abs(o32.cpu().numpy() - ref).max() <= 2e-5 * scale
        o16 = torch.full((n, hw, hw, 128), float("nan"), dtype=torch.bfloat16, device="cuda")
        check(L.snk_conv3x3_bn_mxfp8_act16(xd.data_ptr(), wS.data_ptr(), scd.data_ptr(), shd.data_ptr(), rd.data_ptr(),
                                           o16.data_ptr(), 1, n, hw, hw, 1, _st()))
        got = o16.cpu()
        assert torch.isfinite(got).all()
        want = torch.as_tensor(ref).to(torch.bfloat16)
        err = (got.double() - want.double()).abs()
        assert (err <= 2.0 ** -7 * want.double().abs() + 2e-5 * scale).all() and (got == want).float().mean().item() > 0.99


@pytest.mark.parametrize("golden,blocks", [("states_11x11x4.npz", 4), ("states_19x19x8.npz", 10)])
def test_rect_form_gives_the_same_bits(env, golden, blocks, monkeypatch):
    """the mxfp8 tower through its sub-rectangle layers == through its full layers, bit for bit, on recorded observations"""
    torch, _, net, _ = env
    monkeypatch.setenv("SNK_CONV_ALGO", "mxfp8")
    states = load_golden(golden)["raw"][:256]
    h, w = states.shape[1:3]
    ws = _randomised_bn(net.glorot_uniform_weights((h, w, 3), blocks=blocks, seed=h), 6)
    planes = torch.as_tensor(np.ascontiguousarray(states, np.float32), device="cuda")
    monkeypatch.setenv("SNK_CONV_RECT", "0")
    full = net.QNet(ws, (h, w, 3), max_chunk=8192)
    monkeypatch.setenv("SNK_CONV_RECT", "1")
    rect = net.QNet(ws, (h, w, 3), max_chunk=8192)
    rect.rect_min = 1
    assert full.n_rect == 0 and rect.n_rect >= 2 and rect.backgrounds().dtype == torch.bfloat16 and full.guard_ptr == 0
    q_full = full.forward(planes)
    q_rect = rect.forward(planes)
    for t in rect._ws[("a16", 0)][:3]:
        t.fill_(float("nan"))
    assert torch.isfinite(q_full).all() and torch.equal(q_full, q_rect) and torch.equal(rect.forward(planes), q_full)


@pytest.mark.parametrize("golden,blocks,n,tol_same,tol_f32", [("states_11x11x4.npz", 4, 128, 6e-2, 1e-1),
                                                               ("states_19x19x8.npz", 10, 32, 1e-1, 9e-2)])
def test_whole_net(env, golden, blocks, n, tol_same, tol_f32, monkeypatch):
    """the mxfp8 net (full and sub-rectangle forms, one chunk and small chunks) against the CPU restatement with the same
    rounding points (tests/mxfp8_ref.forward) and against the float32 net (oracle/net_ref.py).  Measured on an MI355X (random
    batch norm): 11x11 / 4 blocks, 128 observations: max |dQ| 3.1e-2 vs the restatement, 5.5e-2 vs the float32 net; 19x19 /
    10 blocks, 32 observations: 5.1e-2 and 4.4e-2.  The bounds are about twice that, the 11x11 one against the float32 net capped
    at 0.1 (past it the form would not be worth shipping).  The restatement is not much closer than
    the float32 net: a last-bit float32 difference (summation order) that flips a bf16 rounding of an activation can move its
    e4m3 code by a whole step (2^-3 relative), so the two drift apart like independent roundings."""
    torch, _, net, _ = env
    from oracle import net_ref
    monkeypatch.setenv("SNK_CONV_ALGO", "mxfp8")
    states = load_golden(golden)["raw"][:n]
    h, w = states.shape[1:3]
    ws = _randomised_bn(net.glorot_uniform_weights((h, w, 3), blocks=blocks, seed=0), 5)
    same = mx.forward(ws, states)
    full = net_ref.forward(ws, states, apply_mask=False)
    for chunk, rect in ((40, "1"), (4096, "1"), (4096, "0")):
        monkeypatch.setenv("SNK_CONV_RECT", rect)
        qn = net.QNet(ws, (h, w, 3), max_chunk=chunk)
        assert qn.act16 == torch.bfloat16 and qn.guard_ptr == 0
        got = qn.forward(torch.as_tensor(np.ascontiguousarray(states, np.float32), device="cuda")).cpu().numpy()
        d_same, d_f32 = np.abs(got - same).max(), np.abs(got - full).max()
        print(f"\n{golden} chunk {chunk} rect {rect}: max|dQ| vs restatement {d_same:.3e}, vs float32 net {d_f32:.3e}")
        assert np.isfinite(got).all()
        assert d_same <= tol_same, d_same
        assert d_f32 <= tol_f32, d_f32


def test_search_root_turn(env, oracle, monkeypatch):
    """one root turn of the configs[4] shape (19x19, 8 snakes) scaled down to 64 games, with the mxfp8 net: moves open,
    Q finite and in [-1, 1], and the recorded states of a sample of games equal the C oracle's observations"""
    torch, se, net, _ = env
    monkeypatch.setenv("SNK_CONV_ALGO", "mxfp8")
    from snake_engine.engine import compact_from_state
    from oracle.obs_key import obstacle_mask
    from utils.agent import Agent
    from utils.alpha_nnet import AlphaNNet
    from utils.mp_game_runner import MPGameRunner
    H = W = 19
    S, games = 8, 64
    old = MPGameRunner.verbose, MPGameRunner.init
    MPGameRunner.verbose, MPGameRunner.init = False, "device"
    try:
        gr = MPGameRunner(H, W, S, 1, games, seed=77)
    finally:
        MPGameRunner.verbose, MPGameRunner.init = old
    eng = gr.engine
    g = torch.Generator(device="cuda").manual_seed(5)
    sub = torch.arange(games, dtype=torch.int32, device="cuda").repeat_interleave(S)
    pairs = torch.stack([sub, torch.arange(S, dtype=torch.int32, device="cuda").repeat(games)], dim=1).contiguous()
    blocked = torch.empty((S * games, 3), dtype=torch.uint8, device="cuda")
    for _ in range(12):                 # a few random open moves: mid-game boards
        eng.observe(pairs, S * games, None, blocked, None)
        r = torch.rand((S * games, 3), device="cuda", generator=g) - 2.0 * blocked.float()
        mv = torch.where(blocked.bool().all(dim=1), torch.ones((), dtype=torch.int64, device="cuda"), r.argmax(dim=1))
        eng.step(mv.to(torch.uint8).reshape(games, S).contiguous())
    over = torch.nonzero(eng.alive().sum(dim=1) <= 1).reshape(-1).to(torch.int32).contiguous()
    if over.numel():
        eng.reset(slots=over)
    alive0 = eng.alive().cpu().numpy().astype(bool)
    pre = eng.export()
    ws = net.glorot_uniform_weights((2 * H - 1, 2 * W - 1, 3), blocks=10, seed=3)
    alice = Agent(AlphaNNet(input_shape=(2 * H - 1, 2 * W - 1, 3), _weights=ws), 2, True, 8, 16, seed=9)
    assert alice.nnet._qnet.conv_algo == "mxfp8"
    seen = []
    make_moves = alice.make_moves

    def spy(games_, ids):
        out = make_moves(games_, ids)
        seen.append((ids, out))
        return out
    alice.make_moves = spy
    gr.run(alice, max_turns=1)
    torch.cuda.synchronize()
    assert len(seen) == 1
    ids, moves = seen[0]
    n_rows = int(alive0.sum())
    assert len(ids) == n_rows == len(alice.records) == len(alice.values)
    V = np.asarray(alice.values[:], np.float32)
    assert np.isfinite(V).all() and (np.abs(V) <= 1.0).all()
    mv_all = np.asarray(moves)
    assert ((mv_all >= 0) & (mv_all <= 2)).all()
    row0 = np.concatenate([[0], np.cumsum(alive0.sum(axis=1))])
    sample = np.arange(0, games, 4)
    rec_idx = np.concatenate([np.arange(row0[gm], row0[gm + 1]) for gm in sample])
    states = alice.records.fetch(rec_idx)
    k = 0
    for gm in sample:
        og = oracle.Game.from_compact(H, W, S, 1, 0.15, compact_from_state(pre[gm]))
        for s in np.flatnonzero(alive0[gm]):
            want = og.make_state(int(s))
            assert states[k].tobytes() == want.tobytes(), f"game {gm} snake {s}: recorded state != Game.make_state"
            bl = obstacle_mask(want)[0]
            mv, v = int(mv_all[rec_idx[k]]), V[rec_idx[k]]
            if not bl.all():
                assert not bl[mv], f"game {gm} snake {s}: chose a blocked move {mv} ({bl})"
                assert (v[bl] == -1.0).all() and (v[~bl] > -1.0).all(), (gm, s, v, bl)
            k += 1
    assert k == len(rec_idx) > 0


def test_bad_arguments_are_refused(env):
    torch, _, net, L = env
    x = torch.zeros((2, 21, 21, 128), dtype=torch.bfloat16, device="cuda")
    o = torch.zeros((2, 21, 21, 128), dtype=torch.bfloat16, device="cuda")
    wS = torch.zeros(net.F16S_WEIGHT_BYTES, dtype=torch.uint8, device="cuda")
    v = torch.zeros(21 * 21 * 128, device="cuda")
    st = _st()
    p, q, sp, vp_ = x.data_ptr(), o.data_ptr(), wS.data_ptr(), v.data_ptr()
    calls = [
        lambda: L.snk_conv3x3_prepare_weights_mxfp8(None, sp, st),
        lambda: L.snk_conv3x3_prepare_weights_mxfp8(vp_, None, st),
        lambda: L.snk_conv3x3_bn_mxfp8_act16(None, sp, vp_, vp_, None, q, 1, 2, 21, 21, 1, st),
        lambda: L.snk_conv3x3_bn_mxfp8_act16(p, None, vp_, vp_, None, q, 1, 2, 21, 21, 1, st),
        lambda: L.snk_conv3x3_bn_mxfp8_act16(p, sp, vp_, vp_, None, None, 1, 2, 21, 21, 1, st),
        lambda: L.snk_conv3x3_bn_mxfp8_act16(p, sp, vp_, vp_, None, q, 1, 0, 21, 21, 1, st),
        lambda: L.snk_conv3x3_bn_mxfp8_act16(p, sp, vp_, vp_, None, q, 1, -1, 21, 21, 1, st),
        lambda: L.snk_conv3x3_bn_mxfp8_act16(p, sp, vp_, vp_, None, q, 1, 1, 1, 200, 1, st),     # wider than the frame holds
        lambda: L.snk_conv3x3_bn_mxfp8_act16_rect(None, sp, vp_, vp_, None, q, vp_, vp_, None, 1, None, 0, None, 2, 21, 21, st),
        lambda: L.snk_conv3x3_bn_mxfp8_act16_rect(p, sp, vp_, vp_, None, q, None, vp_, None, 1, None, 0, None, 2, 21, 21, st),
        lambda: L.snk_conv3x3_bn_mxfp8_act16_rect(p, sp, vp_, vp_, None, q, vp_, vp_, None, 1, None, 0, None, 0, 21, 21, st),
        lambda: L.snk_conv3x3_bn_mxfp8_act16_rect(p, sp, vp_, vp_, None, q, vp_, vp_, None, 1, None, 0, None, 2, 21, 120, st),
        lambda: L.snk_conv3x3_bn_mxfp8_act16_head(None, sp, vp_, vp_, p, vp_, 1.0, 0.0, vp_, 2, 21, 21, st),
        lambda: L.snk_conv3x3_bn_mxfp8_act16_head(p, sp, vp_, vp_, None, vp_, 1.0, 0.0, vp_, 2, 21, 21, st),
        lambda: L.snk_conv3x3_bn_mxfp8_act16_head(p, sp, vp_, vp_, p, vp_, 1.0, 0.0, vp_, 0, 21, 21, st),
        lambda: L.snk_conv3x3_bn_mxfp8_act16_head(p, sp, vp_, vp_, p, vp_, 1.0, 0.0, vp_, 1, 1, 200, st),
        lambda: L.snk_mxfp8_quantize_bf16(None, 4, q, vp_, st),
        lambda: L.snk_mxfp8_quantize_bf16(p, 4, None, vp_, st),
        lambda: L.snk_mxfp8_quantize_bf16(p, 0, q, vp_, st),
        lambda: L.snk_mxfp8_quantize_bf16(p, -3, q, vp_, st),
    ]
    for i, c in enumerate(calls):
        assert c() != 0, i
        assert L.snk_last_error(), i
    torch.cuda.synchronize()
