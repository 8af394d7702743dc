"""The single-pass f16 mode of the training step (TrainStep(conv="f16"), SNK_TRAIN_CONV=f16; alpha_nnet.py:58-59 under Keras fit).

The arithmetic rule (include/snake_engine.h and DESIGN.md section 4 state the same one): an operand v of a tower convolution pass
enters the MFMA as f16(v * s), round to nearest even, s the power of two the split form uses for that tensor (the weight image's
tail words; x_tail / dy_tail of the weight gradient); products are exact in float32, sums are float32, the result is multiplied by
the inverse scales; nothing else is rounded to 16 bits.  So against float64 on operands rounded BY THAT RULE only the float32
accumulation is left, and the split form's own bounds hold (2e-6 for y and dx, 3e-6 for dk, relative to the largest entry);
against the unrounded float64 the error is that of eleven significand bits per operand."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_gpu():
    import torch
    assert torch.cuda.is_available()
    return torch


def rel(a, b):
    return float((a.detach().double() - b.detach().double()).abs().max() / (b.detach().double().abs().max() + 1e-300))


def _tail_of(torch, L, x):
    """{., ., scale, 1 / scale} of a tensor, as the element-wise kernels leave it for the convolution that reads it"""
    from snake_engine.net import F16S_TAIL_OFFSET, F16S_WEIGHT_BYTES
    from snake_engine._lib import check
    image = torch.empty(F16S_WEIGHT_BYTES, dtype=torch.uint8, device="cuda")
    part = torch.empty(L.snk_bn_train_partials(), device="cuda")
    check(L.snk_conv3x3_f16s_input_scale(x.data_ptr(), x.numel(), image.data_ptr(), part.data_ptr(), torch.cuda.current_stream().cuda_stream))
    return image[F16S_TAIL_OFFSET:F16S_TAIL_OFFSET + 16].view(torch.float32).clone()


def _rounded(torch, v, s):
    """the rule: f16(v * s), round to nearest even (torch.float16), as a float64 value of v's magnitude; s is a power of two"""
    return (v * s).to(torch.float16).double() / float(s)


_PASSES = {}


def _three_passes(torch, n, hw, xmag, gmag):
    """the three passes in f16 mode, the forward pass in the split form, and float64 on rounded and on unrounded operands -- once per shape"""
    key = (n, hw, xmag, gmag)
    if key in _PASSES:
        return _PASSES[key]
    import torch.nn.functional as F
    from snake_engine._lib import lib, check
    from snake_engine.net import F16S_TAIL_OFFSET, F16S_WEIGHT_BYTES
    L, st = lib(), torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device="cuda").manual_seed(n)
    x = torch.randn(n, hw, hw, 128, device="cuda", generator=g) * xmag
    k = torch.randn(3, 3, 128, 128, device="cuda", generator=g) * 0.05
    dy = torch.randn(n, hw, hw, 128, device="cuda", generator=g) * gmag
    dy = (dy * (torch.rand(n, hw, hw, 1, device="cuda", generator=g) ** 6)).contiguous()    # a wide spread of magnitudes, as real gradients have
    ones, zeros = torch.ones(128, device="cuda"), torch.zeros(128, device="cuda")
    image = torch.empty(F16S_WEIGHT_BYTES, dtype=torch.uint8, device="cuda")
    image_b = torch.empty_like(image)
    tx, tdy = _tail_of(torch, L, x), _tail_of(torch, L, dy)
    y, dx, y_split = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
    check(L.snk_conv3x3_prepare_weights_f16s_train(k.data_ptr(), image.data_ptr(), tx.data_ptr(), 0, None, st))
    check(L.snk_conv3x3_bn_f16(x.data_ptr(), image.data_ptr(), ones.data_ptr(), zeros.data_ptr(), None, y.data_ptr(), n, hw, hw, 0, st))
    check(L.snk_conv3x3_bn_f16s(x.data_ptr(), image.data_ptr(), ones.data_ptr(), zeros.data_ptr(), None, y_split.data_ptr(), n, hw, hw, 0, st))
    check(L.snk_conv3x3_prepare_weights_f16s_train(k.data_ptr(), image_b.data_ptr(), tdy.data_ptr(), 1, image.data_ptr(), st))
    check(L.snk_conv3x3_bn_f16(dy.data_ptr(), image_b.data_ptr(), ones.data_ptr(), zeros.data_ptr(), None, dx.data_ptr(), n, hw, hw, 0, st))
    part = torch.empty(L.snk_conv3x3_wgrad_partials(hw, hw), device="cuda")
    dk = torch.empty(3, 3, 128, 128, device="cuda")
    check(L.snk_conv3x3_wgrad_f16(x.data_ptr(), dy.data_ptr(), tx.data_ptr(), tdy.data_ptr(), part.data_ptr(), dk.data_ptr(), n, hw, hw, st))
    # the forward form the step uses: the same convolution with the batch-norm sums taken in its epilogue
    center = torch.randn(128, device="cuda", generator=g) * xmag
    cpart = torch.empty(L.snk_conv3x3_stats_partials(n, hw, hw), device="cuda")
    sums = torch.empty(256, dtype=torch.float64, device="cuda")
    y2 = torch.empty_like(x)
    check(L.snk_conv3x3_f16_stats(x.data_ptr(), image.data_ptr(), y2.data_ptr(), center.data_ptr(), cpart.data_ptr(), sums.data_ptr(), n, hw, hw, st))
    torch.cuda.synchronize()
    tails = [im[F16S_TAIL_OFFSET:F16S_TAIL_OFFSET + 32] for im in (image, image_b)]
    assert all(int(t[16:20].view(torch.int32)) == 0 for t in tails), "a range flag is set: an operand was clamped"
    # the scales as the library wrote them: weights tail[1], input tail[2] (the two images share the weight scale)
    tw, tb = tails[0][:16].view(torch.float32), tails[1][:16].view(torch.float32)
    ws, xs, dys = float(tw[1]), float(tw[2]), float(tb[2])
    assert ws == float(tb[1]) and xs == float(tx[2]) and dys == float(tdy[2]) and float(tw[0]) * ws == 1.0

    def f64(xv, kv, dyv):
        x64 = xv.permute(0, 3, 1, 2).requires_grad_(True)
        k64 = kv.requires_grad_(True)
        y64 = F.conv2d(x64, k64.permute(3, 2, 0, 1), padding=1)
        dx64, dk64 = torch.autograd.grad(y64, (x64, k64), dyv.permute(0, 3, 1, 2))
        return y64.detach().permute(0, 2, 3, 1), dx64.permute(0, 2, 3, 1), dk64
    ref_r = f64(_rounded(torch, x, xs), _rounded(torch, k, ws), _rounded(torch, dy, dys))
    y_exact = F.conv2d(x.double().permute(0, 3, 1, 2), k.double().permute(3, 2, 0, 1), padding=1).permute(0, 2, 3, 1)
    _PASSES[key] = dict(y=y, dx=dx, dk=dk, y2=y2, y_split=y_split, sums=sums, center=center, ref=ref_r, y_exact=y_exact)
    return _PASSES[key]


@pytest.mark.parametrize("n,hw,xmag,gmag", [(64, 21, 1.0, 1.0), (48, 21, 30.0, 1e-6), (5, 13, 1e-3, 50.0), (3, 37, 1.0, 1e-4),
                                           (41, 37, 1.0, 1.0)])      # the 19x19 batched plan: 9 blocks of 5 / 4 tiles (tests/conv_plan_ref.py)
def test_three_passes_match_float64_on_the_rounded_operands(torch_gpu, n, hw, xmag, gmag):
    """forward and input gradient on k_conv3x3_f16s<SPLIT = false>, weight gradient on k_wgrad2_f16s<HI> (the two compile-time-width
    forms and the generic one; image counts that leave most of the 128 image groups empty; both ends of the scale range)"""
    torch = torch_gpu
    r = _three_passes(torch, n, hw, xmag, gmag)
    y64, dx64, dk64 = r["ref"]
    e = (rel(r["y"], y64), rel(r["dx"], dx64), rel(r["dk"], dk64))
    print(f"f16 three passes n={n} hw={hw}: rel y {e[0]:.3g} dx {e[1]:.3g} dk {e[2]:.3g}")
    assert e[0] < 2e-6 and e[1] < 2e-6, e
    assert e[2] < 3e-6, e
    assert torch.equal(r["y2"], r["y"])                     # the form with the sums == the bare f16 convolution, bit for bit
    d = r["y"].double().reshape(-1, 128) - r["center"].double()
    assert rel(r["sums"][:128], d.sum(dim=0)) < 1e-5 and rel(r["sums"][128:], (d * d).sum(dim=0)) < 1e-6


def test_the_mode_multiplies_the_hi_halves_only_and_keeps_the_scales(torch_gpu):
    """eleven significand bits per operand: about 5e-4 per product before averaging over 1 152 terms.  An error below the floor means
    the lo halves are still multiplied, one above the ceiling that an operand lost its scale."""
    torch = torch_gpu
    r = _three_passes(torch, 64, 21, 1.0, 1.0)
    assert not torch.equal(r["y"], r["y_split"])
    e, e_split = rel(r["y"], r["y_exact"]), rel(r["y_split"], r["y_exact"])
    print(f"f16 against unrounded float64: rel y {e:.3g} (split form {e_split:.3g})")
    assert 1e-5 < e < 2e-3, e
    assert e_split < 2e-6


def _problem(n, blocks, hw, seed):
    import torch
    from snake_engine import net
    rs = np.random.RandomState(seed)
    X = torch.as_tensor(rs.rand(n, hw, hw, 3).astype(np.float32), device="cuda")
    Y = torch.as_tensor(np.tanh(rs.randn(n, 3)).astype(np.float32), device="cuda")
    ws = net.glorot_uniform_weights((hw, hw, 3), blocks=blocks, seed=6)
    for l in range(2 + 2 * blocks):                         # batch-norm parameters away from 1 / 0, some scales NEGATIVE
        g = ws[5 * l + 1] * (0.6 + 0.8 * rs.rand(*ws[5 * l + 1].shape))
        g[::7] *= -1.0
        ws[5 * l + 1] = g.astype(np.float32)
        ws[5 * l + 2] = (0.3 * rs.randn(*ws[5 * l + 2].shape)).astype(np.float32)
    return ws, X, Y


@pytest.mark.parametrize("switch", ["_DEFER_BN", "_RES_MASK", "_DEFER_STEM"])
@pytest.mark.parametrize("n,blocks,hw", [(6, 1, 13), (5, 2, 21)])
def test_deferred_batch_norm_mask_bytes_and_deferred_stem_under_f16(torch_gpu, monkeypatch, switch, n, blocks, hw):
    """the twin runs of the split form's tests (SNK_TRAIN_DEFER_BN=0, SNK_TRAIN_RES_MASK=0, SNK_TRAIN_DEFER_STEM=0) with
    conv="f16": both runs round the same operands, only the summation order (and the input range's power of two) differs"""
    from snake_engine import train_step
    ws, X, Y = _problem(n, blocks, hw, 100 + n)
    if switch == "_RES_MASK":
        monkeypatch.setattr(train_step, "_DEFER_STEM", False)   # (the deferred stem exists with the masked shortcut only: one change per twin)
    runs = {}
    for on in (False, True):
        monkeypatch.setattr(train_step, switch, on)
        ts = train_step.TrainStep(ws, (hw, hw, 3), n, "cuda", conv="f16")
        assert {"_DEFER_BN": ts.defer, "_RES_MASK": ts.res_mask, "_DEFER_STEM": ts.defer_stem}[switch] == on
        q = ts.forward(X, Y, n).clone()
        ts.backward(Y, n)
        runs[on] = (q, ts.gradients(), ts.weights())
    (q0, g0, w0), (q1, g1, w1) = runs[False], runs[True]
    dq = float((q0 - q1).abs().max())
    dg = max(np.abs(g0[j] - g1[j]).max() / max(np.abs(g0[j]).max(), 1e-12) for j in g0)
    dw = max(np.abs(u - v).max() / max(np.abs(u).max(), 1e-12) for u, v in zip(w0, w1))
    print(f"f16 twin {switch} n={n} blocks={blocks} hw={hw}: dQ {dq:.3g} gradients {dg:.3g} weights {dw:.3g}")
    assert dq <= 2e-6 and dg <= 2e-5 and dw <= 1e-6, (dq, dg, dw)


def test_input_gradient_epilogue_reads_nothing_behind_the_last_image_in_f16_mode(torch_gpu, monkeypatch):
    """the construction of the split form's test, once, at (3, 21): every tensor the input-gradient epilogue reads is followed by NaN
    (mask bytes: all ones), the output by a sentinel"""
    torch = torch_gpu
    from snake_engine import net, train_step
    from snake_engine._lib import lib, check
    from snake_engine.train_step import _p
    n, hw = 3, 21
    rs = np.random.RandomState(7 * n + hw)
    X = torch.as_tensor(rs.rand(n, hw, hw, 3).astype(np.float32), device="cuda")
    Y = torch.as_tensor(np.tanh(rs.randn(n, 3)).astype(np.float32), device="cuda")
    ws = net.glorot_uniform_weights((hw, hw, 3), blocks=2, seed=4)
    monkeypatch.setattr(train_step, "_DEFER_BN", False)
    ts = train_step.TrainStep(ws, (hw, hw, 3), n, "cuda", conv="f16")   # n == max_rows: nothing of the step's own lies behind image n - 1
    ts.forward(X, Y, n)
    ts.backward(Y, n)
    L, st = lib(), torch.cuda.current_stream().cuda_stream
    act, l = n * hw * hw * 128, 2
    slack = 64 * 128                                                # 64 rows: more than any block reaches past its image

    def padded(t, count, fill):
        buf = torch.full((count + (slack if t.dtype != torch.uint8 else slack // 4),), fill, dtype=t.dtype, device="cuda")
        buf[:count] = t.reshape(-1)[:count]
        return buf
    nan = float("nan")
    dY, res = padded(ts.dY, act, nan), padded(ts.gres, act, nan)
    y, mask = padded(ts.y[l - 1], act, nan), padded(ts.relu_mask[l - 1], act // 4, 255)
    rmask = padded(ts.relu_mask[l], act // 4, 255)
    for masked in (False, True):
        outs = []
        for pad in (False, True):
            out = torch.full((act + slack,), 12345.0, device="cuda")
            sums = torch.zeros(256, dtype=torch.float64, device="cuda")
            a = (dY, res, y, mask, rmask) if pad else (ts.dY, ts.gres, ts.y[l - 1], ts.relu_mask[l - 1], ts.relu_mask[l])
            if masked:
                check(L.snk_conv3x3_f16_igrad_stats_masked_res(_p(a[0]), _p(ts.img_b), _p(a[1]), _p(a[4]), _p(out), _p(a[2]), _p(a[3]),
                                                               _p(ts.mean[l - 1]), _p(ts.inv[l - 1]), _p(ts.cv_partials), _p(sums), n, hw, hw, st))
            else:
                check(L.snk_conv3x3_f16_igrad_stats(_p(a[0]), _p(ts.img_b), _p(a[1]), _p(out), _p(a[2]), _p(a[3]), _p(ts.mean[l - 1]),
                                                    _p(ts.inv[l - 1]), _p(ts.cv_partials), _p(sums), n, hw, hw, st))
            torch.cuda.synchronize()
            outs.append((out.clone(), sums.clone()))
        (o0, s0), (o1, s1) = outs
        assert torch.isfinite(s1).all() and torch.isfinite(o1[:act]).all()
        assert torch.equal(o0[:act], o1[:act]) and torch.equal(s0, s1)
        assert (o1[act:] == 12345.0).all() and (o0[act:] == 12345.0).all(), "the epilogue stored behind the last image"
        assert float(s1.abs().max()) > 0


# One whole step in f16 mode against the float64 autograd graph at (n, blocks, hw) = (8, 1, 13), the float64 run's ReLU masks imposed
# on the backward pass.  The errors below are MEASURED (one MI355X, this seed; the step repeats bit for bit) and asserted at three
# times their value, to leave room for another seed's rounding.  They are those of eleven significand bits per operand through
# four convolution layers: the split form's bounds for the same step are 1e-5 (Q, loss) and 1e-4 (gradients).
MEASURED_Q = 1.28e-3                                        # max |Q - Q64|
MEASURED_LOSS = 3.34e-4                                     # |mse - mse64| / mse64
MEASURED_GRAD = {22: 9.54e-4, 11: 8.55e-4, 2: 8.09e-4, 23: 7.60e-4, 12: 7.38e-4, 1: 6.83e-4, 5: 6.69e-4, 20: 6.41e-4, 15: 6.32e-4,
                 21: 5.54e-4, 10: 5.44e-4, 6: 5.22e-4, 7: 5.22e-4, 0: 4.52e-4, 16: 2.29e-4, 17: 1.29e-4}     # Keras list index: relative to the tensor's largest entry


def test_one_whole_step_in_f16_mode_against_float64(torch_gpu):
    torch = torch_gpu
    from snake_engine import net
    from snake_engine.train_step import TrainStep
    from test_train_ops_gpu import _net64
    n, blocks, hw = 8, 1, 13
    rs = np.random.RandomState(5 + n)
    X = rs.rand(n, hw, hw, 3).astype(np.float32)
    Y = np.tanh(rs.randn(n, 3)).astype(np.float32)
    ws = net.glorot_uniform_weights((hw, hw, 3), blocks=blocks, seed=9)
    for l in range(2 + 2 * blocks):                         # batch-norm parameters away from their initial 1 / 0
        ws[5 * l + 1] = (ws[5 * l + 1] * (0.6 + 0.8 * rs.rand(*ws[5 * l + 1].shape))).astype(np.float32)
        ws[5 * l + 2] = (0.2 * rs.randn(*ws[5 * l + 2].shape)).astype(np.float32)
    loss64, g64, pre, q64, n_conv = _net64(torch, ws, X, Y)
    ts = TrainStep(ws, (hw, hw, 3), n, "cuda", conv="f16")
    x, y = torch.as_tensor(X, device="cuda"), torch.as_tensor(Y, device="cuda")
    q = ts.forward(x, y, n)
    dq = float((q.double() - q64).abs().max())
    dloss = abs(float(ts.G[ts.n_params]) - loss64) / loss64
    sign = lambda z: torch.where(z > 0, 1.0, -1.0).float().contiguous()
    for l in range(n_conv - 1):                             # the 128-channel layers: [n, C, h, w] float64 -> channels-last rows
        ts.mask_override[l] = sign(pre[l].permute(0, 2, 3, 1)).reshape(-1)
    ts.mask_override["h"] = sign(pre[n_conv - 1].permute(0, 2, 3, 1)).reshape(-1)
    ts.mask_override["d1"] = sign(pre["d1"]).reshape(-1)
    ts.backward(y, n)
    got = ts.gradients()
    worst = {j: float((torch.as_tensor(got[j], device="cuda").double() - ref).abs().max() / (ref.abs().max() + 1e-300)) for j, ref in g64.items()}
    print(f"f16 whole step: |dQ| {dq:.3g} loss {dloss:.3g} gradients {sorted(worst.items(), key=lambda kv: -kv[1])}")
    assert dq < 3 * MEASURED_Q                              # measured: 1.28e-3
    assert dloss < 3 * MEASURED_LOSS                        # measured: 3.34e-4
    assert set(worst) == set(MEASURED_GRAD)
    for j, e in worst.items():
        assert e < 3 * MEASURED_GRAD[j], (j, e)             # measured: 1.29e-4 (Dense bias) .. 9.54e-4, see MEASURED_GRAD


def test_fit_in_f16_mode_tracks_fit_with_library_operators(torch_gpu):
    """the construction of test_fit_on_the_kernels_tracks_fit_with_library_operators with SNK_TRAIN_CONV=f16 against
    SNK_TRAIN_CONV=torch, the same bounds"""
    import os
    import subprocess
    import sys
    import tempfile
    from conftest import REPO
    code = r'''
import sys, numpy as np, torch
sys.path[:0] = [r"%s", r"%s/alphasnake-zero_amd"]
from snake_engine import net
from utils import trainer_torch
rs = np.random.RandomState(3)
X = rs.rand(512, 21, 21, 3).astype(np.float32); Y = np.tanh(rs.randn(512, 3)).astype(np.float32)
ws = net.glorot_uniform_weights((21, 21, 3), blocks=4, seed=5)
out = trainer_torch.fit(ws, (21, 21, 3), X, Y, 3, 128, ([4, 8], [1e-3, 2.5e-4, 0.0]), seed=11, verbose=False)
q = trainer_torch._Net(out, torch.device("cuda")).forward(torch.as_tensor(X[:96], device="cuda"), False).detach().cpu().numpy()
np.savez(sys.argv[1], hist=np.array(trainer_torch.fit.last_history), q=q, mode=trainer_torch.fit.last_mode)
''' % (REPO, REPO)
    res = {}
    with tempfile.TemporaryDirectory() as d:
        for mode in ("f16", "torch"):
            path = os.path.join(d, mode + ".npz")
            r = subprocess.run([sys.executable, "-c", code, path], env=dict(os.environ, SNK_TRAIN_CONV=mode), capture_output=True,
                               text=True, timeout=600)
            assert r.returncode == 0, r.stderr[-2000:]
            z = np.load(path)
            res[mode] = (z["hist"], z["q"], str(z["mode"]))
    (h_a, q_a, m_a), (h_b, q_b, m_b) = res["f16"], res["torch"]
    assert (m_a, m_b) == ("kernels-f16", "autograd")
    print(f"f16 fit: loss history {h_a} against {h_b}; |dQ| max {np.abs(q_a - q_b).max():.3g} mean {np.abs(q_a - q_b).mean():.3g}")
    assert len(h_a) == 3 and h_a[2] < h_a[0]                                    # it trains
    assert np.abs(h_a - h_b).max() / np.abs(h_b).max() < 1e-2, (h_a, h_b)
    assert np.abs(q_a - q_b).max() < 5e-2 and np.abs(q_a - q_b).mean() < 5e-3, (np.abs(q_a - q_b).max(), np.abs(q_a - q_b).mean())
