"""Every launch form of the inference head (csrc/net.hip: k_head behind snk_head_f32, k_head_dense<16 / 8 / 4> behind
snk_head_dense_f32) against the float64 model tests/stem_head_ref.py.  The head reads no environment: everything runs in-process.

Bound: |q - ref| <= 2e-6 (what tests/test_net_gpu.py::test_stem_and_head_layers uses), masked entries exactly -1.0, and the row
of NaN behind q still NaN.  Inputs are placed so that a wrong kernel cannot hide: the 1x1 stage's shift b1 is the negated median of
its pre-activation (half of h1 clamped, asserted on the reference as a share in [0.3, 0.7]; a single pixel of a single state
has no share, it is kept positive), and fc2_b moves state 0's first pre-tanh value to 0.05 (the linear part of the tanh, where an
error of the dot products arrives undamped) and its second to 4.5 (the saturated part), asserted on the reference.
Each test prints `fig <entry> <case> <largest |q - ref|>` before it asserts."""
import ctypes as C
import functools

import numpy as np
import pytest

import stem_head_ref as R

pytestmark = pytest.mark.gpu
TOL_Q = 2e-6
NAN = float("nan")

# snk_head_f32 (n, H, W)
HEAD_SHAPES = [(1, 1, 1),         # gap 8: HW < 4, three wavefronts own no pixel; the second half-sum is empty
               (2, 1, 2),         # gap 8: HW < 4, even: mid = 1
               (3, 1, 3),         # gap 8: HW < 4, odd
               (2, 1, 5),         # one wavefront owns two pixels
               (5, 20, 20),       # gap 8: even HW, the two half-sums meet at mid = 200
               (3, 21, 21),
               (2, 37, 37)]
# snk_head_dense_f32 (n, H, W)
DENSE_SHAPES = [(1, 1, 5), (17, 1, 5),                                   # gap 7: <16>, HW < 8: the tail loop only
                (1, 21, 21), (16, 21, 21), (17, 21, 21), (37, 21, 21),   # <16>, HW % 8 = 1
                (9, 20, 20),                                             # <16>, HW % 8 = 0: no tail
                (1, 37, 37), (8, 37, 37),                                # gap 7: <8>, the 19 x 19 board's production head
                (5, 37, 37), (13, 37, 37),                               # gap 7: <8>, a last block whose states straddle the two thread halves
                (1, 45, 45), (3, 45, 45), (7, 45, 45),                   # gap 7: <4>
                (2, 62, 64)]                                             # gap 7: <4>, 4 (3968 + 128) 4 = 65 536 bytes exactly: accepted
DENSE_REFUSED = (2, 63, 63)                                              # gap 7: 4 (3969 + 128) 4 = 65 552 bytes: refused


def _f32(t):
    return np.ascontiguousarray(t.numpy(), dtype=np.float32)


def _mask(g, n):
    import torch
    m = (torch.rand(n, 3, generator=g) < 0.35).to(torch.uint8).numpy()
    m[0, 0], m[0, 2] = 0, 1              # at least one move kept (the one placed in the tanh's linear part) and one overwritten
    return m


def _fc2(g, h1, fc1_w, fc1_b):
    """fc2_w = randn * 0.1; fc2_b places state 0's pre-tanh values at 0.05 and 4.5 (asserted by the caller on the reference)"""
    import torch
    fc2_w = _f32(torch.randn(R.C, 3, generator=g) * 0.1)
    v0 = R.head_pre_tanh(h1[:1], fc1_w, fc1_b, fc2_w, np.zeros(3))[0]
    fc2_b = np.float32([0.05 - v0[0], 4.5 - v0[1], float(torch.randn(1, generator=g)) * 0.1])
    return fc2_w, fc2_b


@functools.lru_cache(maxsize=None)
def head_case(n, H, W):
    """operands (float32 NumPy), the mask, and the float64 reference with and without the mask: computed once per shape"""
    import torch
    g = torch.Generator().manual_seed(10000 * n + 100 * H + W)
    HW = H * W
    d = dict(act=_f32(torch.randn(n, H, W, R.C, generator=g)), w1=_f32(torch.randn(R.C, generator=g) * 0.1), s1=0.7)
    z = np.sort(((R.f64(d["act"]).reshape(-1, R.C) @ R.f64(d["w1"])) * np.float64(np.float32(0.7))))
    d["b1"] = float(np.float32(-(z[z.size // 2 - 1] + z[z.size // 2]) / 2)) if z.size > 1 else float(np.float32(0.25 - z[0]))
    d["fc1_w"] = _f32(torch.randn(HW, R.C, generator=g) * 0.05)
    d["fc1_b"] = _f32(torch.randn(R.C, generator=g) * 0.1)
    s1 = float(np.float32(0.7))
    h1, _ = R.head(d["act"], d["w1"], s1, d["b1"], d["fc1_w"], d["fc1_b"], np.zeros((R.C, 3)), np.zeros(3))
    d["fc2_w"], d["fc2_b"] = _fc2(g, h1, d["fc1_w"], d["fc1_b"])
    d["mask"] = _mask(g, n)
    d["h1"], d["q"] = R.head(d["act"], d["w1"], s1, d["b1"], d["fc1_w"], d["fc1_b"], d["fc2_w"], d["fc2_b"])
    d["q_masked"] = R.head(d["act"], d["w1"], s1, d["b1"], d["fc1_w"], d["fc1_b"], d["fc2_w"], d["fc2_b"], d["mask"])[1]
    d["pre"] = R.head_pre_tanh(d["h1"], d["fc1_w"], d["fc1_b"], d["fc2_w"], d["fc2_b"])
    d["clamped"] = float((d["h1"] == 0).mean())
    return d


@functools.lru_cache(maxsize=None)
def dense_case(n, H, W):
    """h1 = relu(randn) given directly; the Dense kernel randn / sqrt(HW), so that h2 is of order 1 on every canvas"""
    import torch
    g = torch.Generator().manual_seed(20000 * n + 100 * H + W)
    HW = H * W
    d = dict(h1=_f32(torch.randn(n, HW, generator=g).clamp_min(0)), fc1_w=_f32(torch.randn(HW, R.C, generator=g) / HW ** 0.5),
             fc1_b=_f32(torch.randn(R.C, generator=g) * 0.1))
    d["fc2_w"], d["fc2_b"] = _fc2(g, R.f64(d["h1"]), d["fc1_w"], d["fc1_b"])
    d["mask"] = _mask(g, n)
    d["q"] = R.head_dense(d["h1"], d["fc1_w"], d["fc1_b"], d["fc2_w"], d["fc2_b"])
    d["q_masked"] = R.head_dense(d["h1"], d["fc1_w"], d["fc1_b"], d["fc2_w"], d["fc2_b"], d["mask"])
    d["pre"] = R.head_pre_tanh(d["h1"], d["fc1_w"], d["fc1_b"], d["fc2_w"], d["fc2_b"])
    return d


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available()
    from snake_engine._lib import lib
    return torch, lib()


def _dev(torch, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def run_head(gpu, d, n, H, W, masked):
    torch, L = gpu
    from snake_engine._lib import check
    t = _dev(torch, d["act"], d["w1"], d["fc1_w"], d["fc1_b"], d["fc2_w"], d["fc2_b"], d["mask"])
    q = torch.full((n + 1, 3), NAN, device="cuda")
    check(L.snk_head_f32(t[0].data_ptr(), t[1].data_ptr(), C.c_float(d["s1"]), C.c_float(d["b1"]), t[2].data_ptr(), t[3].data_ptr(),
                         t[4].data_ptr(), t[5].data_ptr(), t[6].data_ptr() if masked else None, q.data_ptr(), n, H, W,
                         torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return q.cpu().double().numpy()


def run_dense(gpu, d, h1, n, H, W, masked):
    torch, L = gpu
    from snake_engine._lib import check
    t = _dev(torch, h1, d["fc1_w"], d["fc1_b"], d["fc2_w"], d["fc2_b"], d["mask"])
    q = torch.full((n + 1, 3), NAN, device="cuda")
    check(L.snk_head_dense_f32(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), t[4].data_ptr(),
                               t[5].data_ptr() if masked else None, q.data_ptr(), n, H, W, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return q.cpu().double().numpy()


def hold(entry, case, got, d, n, masked):
    ref = d["q_masked"] if masked else d["q"]
    assert (np.abs(d["pre"]) < 0.1).any() and (np.abs(d["pre"]) > 4).any()          # both parts of the tanh are in the reference
    assert (d["q"] > -1.0).all()                                                    # -1.0 is the overwrite's alone
    assert np.isnan(got[n]).all(), "the row behind q was written"
    assert np.isfinite(got[:n]).all()
    err = float(np.abs(got[:n] - ref).max())
    print(f"fig {entry} {case} {err:.3e}")
    assert err <= TOL_Q, (entry, case, err)
    if masked:
        assert d["mask"].any() and (got[:n][d["mask"] != 0] == -1.0).all()
        assert (got[:n][d["mask"] == 0] > -1.0).all()
    else:
        assert (got[:n] > -1.0).all()                                               # gap 7 / 8: mask == NULL overwrites nothing


@pytest.mark.parametrize("masked", [True, False], ids=["mask", "nomask"])
@pytest.mark.parametrize("n,H,W", HEAD_SHAPES)
def test_head_f32(gpu, n, H, W, masked):
    d = head_case(n, H, W)
    if n * H * W > 1:
        assert 0.3 <= d["clamped"] <= 0.7, d["clamped"]
    else:
        assert d["clamped"] == 0.0 and abs(d["h1"][0, 0] - 0.25) < 1e-6
    hold("snk_head_f32", f"{n}x{H}x{W}", run_head(gpu, d, n, H, W, masked), d, n, masked)


@pytest.mark.parametrize("masked", [True, False], ids=["mask", "nomask"])
@pytest.mark.parametrize("n,H,W", DENSE_SHAPES)
def test_head_dense_f32(gpu, n, H, W, masked):
    assert R.head_dense_states_per_block(H, W) == {1 * 5: 16, 21 * 21: 16, 20 * 20: 16, 37 * 37: 8, 45 * 45: 4, 62 * 64: 4}[H * W]
    d = dense_case(n, H, W)
    hold("snk_head_dense_f32", f"{n}x{H}x{W}", run_dense(gpu, d, d["h1"], n, H, W, masked), d, n, masked)


def test_head_dense_f32_refuses_what_does_not_fit_64k(gpu):
    torch, L = gpu
    from snake_engine._lib import EngineError
    n, H, W = DENSE_REFUSED
    assert R.head_dense_states_per_block(H, W) == 0 and R.head_dense_states_per_block(62, 64) == 4
    g = torch.Generator().manual_seed(6363)
    d = dict(fc1_w=_f32(torch.randn(H * W, R.C, generator=g) / (H * W) ** 0.5), fc1_b=np.zeros(R.C, np.float32),
             fc2_w=_f32(torch.randn(R.C, 3, generator=g) * 0.1), fc2_b=np.zeros(3, np.float32), mask=np.zeros((n, 3), np.uint8))
    h1 = _f32(torch.randn(n, H * W, generator=g).clamp_min(0))
    t = _dev(torch, h1, d["fc1_w"], d["fc1_b"], d["fc2_w"], d["fc2_b"], d["mask"])
    q = torch.full((n + 1, 3), NAN, device="cuda")
    from snake_engine._lib import check
    with pytest.raises(EngineError):                    # the host code refuses before any launch
        check(L.snk_head_dense_f32(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), t[4].data_ptr(),
                                   t[5].data_ptr(), q.data_ptr(), n, H, W, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert bool(torch.isnan(q).all())


@pytest.mark.parametrize("n,H,W", HEAD_SHAPES)
def test_head_f32_and_head_dense_f32_agree(gpu, n, H, W):
    """snk_head_f32 on the activations and snk_head_dense_f32 on the reference's h1 rounded to float32: each is within 2e-6 of the
    same reference, so they agree within 4e-6"""
    assert R.head_dense_states_per_block(H, W) > 0
    d = head_case(n, H, W)
    a = run_head(gpu, d, n, H, W, True)
    b = run_dense(gpu, d, d["h1"].astype(np.float32), n, H, W, True)
    assert np.isnan(a[n]).all() and np.isnan(b[n]).all()
    err = float(np.abs(a[:n] - b[:n]).max())
    print(f"fig head_vs_dense {n}x{H}x{W} {err:.3e}")
    assert err <= 2 * TOL_Q, err
    assert (a[:n][d["mask"] != 0] == -1.0).all() and (b[:n][d["mask"] != 0] == -1.0).all()
