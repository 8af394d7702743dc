"""tests/train_head_ref.py, the float64 model tests/test_train_head_gpu.py holds the training head's kernels to, proven without a
GPU: against float64 autograd of the same graph (1x1 convolution -> one-channel batch norm -> ReLU -> Flatten -> Dense(128) ->
ReLU -> Dense(3) -> tanh -> sum (q - t)^2 norm, alpha_nnet.py:49-54 under Keras fit), the mask byte convention by hand, the
entry points' limits for every case, and the 2^24 headroom that makes the integer cases exact in float32 in any order."""
import numpy as np
import pytest

import train_head_ref as R

REL = 1e-12


def close(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return got.shape == ref.shape and float(np.abs(got - ref).max()) <= REL * float(np.abs(ref).max())


def _graph(n, H, W, seed, batch_stats):
    """the reference's three backward functions chained, and autograd of the same graph.  batch_stats False: mean / inv given and
    held constant (abc = (gamma inv, 0, 0)); True: they are the batch's own, so autograd also goes through them (the b and c terms)"""
    import torch
    HW, rows = H * W, n * H * W
    rs = np.random.RandomState(seed)
    a = np.maximum(rs.randn(rows, R.C), 0.0)
    w1x1 = rs.randn(R.C) * 0.1
    W1, b1 = rs.randn(HW, R.C) / np.sqrt(HW), rs.randn(R.C) * 0.1
    W2, b2 = rs.randn(R.C, 3) * 0.15, rs.randn(3) * 0.1
    target = np.tanh(rs.randn(n, 3))
    gamma, beta, eps, norm = 1.2, 0.15, 1e-3, 1.0 / (3 * n)
    y_last = rs.randn(rows, R.C)
    mean_last, inv_last = rs.randn(R.C) * 0.1, rs.rand(R.C) + 0.5
    mask_last = rs.randint(0, 16, size=(rows, R.C // 4)).astype(np.uint8)

    t = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in
         dict(a=a, w1x1=w1x1, W1=W1, b1=b1, W2=W2, b2=b2).items()}
    z_t = t["a"] @ t["w1x1"]
    if batch_stats:
        mean_t = z_t.mean()
        inv_t = 1.0 / torch.sqrt(((z_t - mean_t) ** 2).mean() + eps)
    else:
        mean_t, inv_t = torch.tensor(0.1, dtype=torch.float64), torch.tensor(1.7, dtype=torch.float64)
    u_t = (((z_t - mean_t) * inv_t) * gamma + beta).reshape(n, HW)
    u_t.retain_grad()
    a_t_grad_probe = t["a"]
    pre1_t = torch.relu(u_t) @ t["W1"] + t["b1"]
    q_t = torch.tanh(torch.relu(pre1_t) @ t["W2"] + t["b2"])
    loss = ((q_t - torch.tensor(target)) ** 2).sum() * norm
    loss.backward()

    mean, inv = float(mean_t.detach()), float(inv_t.detach())
    scale, shift = gamma * inv, beta - mean * gamma * inv
    c = R.conv1x1_sums(a, w1x1, None)
    z = c["z"].reshape(n, HW)
    f = R.dense_fwd(z, scale, shift, W1, b1, W2, b2, target, norm)
    b = R.dense_bwd(f["q"], target, f["d1"], f["h"], f["pre_h"], f["pre1"], z, mean, inv, W1, W2, norm)
    abc = (gamma * inv, b["gsums"][0] / rows, b["gsums"][1] / rows) if batch_stats else (gamma * inv, 0.0, 0.0)
    e = R.conv1x1_bwd(b["g"], z, mean, inv, abc, a, w1x1, y_last, mask_last, mean_last, inv_last)
    auto = dict(loss=float(loss.detach()), q=q_t.detach().numpy(), g=u_t.grad.numpy(), dW1=t["W1"].grad.numpy(), db1=t["b1"].grad.numpy(),
                dW2=t["W2"].grad.numpy(), db2=t["b2"].grad.numpy(), da=a_t_grad_probe.grad.numpy(), dw1x1=t["w1x1"].grad.numpy())
    return auto, c, f, b, e, dict(y_last=y_last, mean_last=mean_last, inv_last=inv_last, mask_last=mask_last, z=z, mean=mean, inv=inv)


@pytest.mark.parametrize("batch_stats", [False, True])
@pytest.mark.parametrize("n,H,W", [(3, 3, 5), (5, 4, 6)])                 # HW = 15 (odd) and 24
def test_the_reference_equals_float64_autograd_of_the_same_graph(n, H, W, batch_stats):
    auto, c, f, b, e, x = _graph(n, H, W, 7 * n + H, batch_stats)
    assert close(f["q"], auto["q"]) and abs(f["sq_err"] - auto["loss"]) <= REL * abs(auto["loss"])
    assert close(b["g"], auto["g"])                                       # the gradient at the batch norm's output, ReLU applied
    assert close(b["dW1"], auto["dW1"])
    assert close(b["small"][:384].reshape(R.C, 3), auto["dW2"])
    assert close(b["small"][384:387], auto["db2"]) and close(b["small"][387:], auto["db1"])
    assert close(e["da"], auto["da"]) and close(e["dw1x1"], auto["dw1x1"])
    # the masks really were the signs of the float64 pre-activations, both ways
    assert (f["h"] > 0).any() and (f["h"] == 0).any() and (f["d1"] > 0).any() and (f["d1"] == 0).any()
    # the two sums the batch norm's backward starts from, and those of the last tower layer, written out once more
    zhat = (x["z"] - x["mean"]) * x["inv"]
    assert close(b["gsums"], [auto["g"].sum(), (auto["g"] * zhat).sum()])
    bits = np.zeros((n * H * W, R.C), dtype=bool)
    for r in range(bits.shape[0]):
        for ch in range(R.C):
            bits[r, ch] = (int(x["mask_last"][r, ch // 4]) >> (ch % 4)) & 1
    gp = np.where(bits, auto["da"], 0.0)
    xh = (x["y_last"] - x["mean_last"]) * x["inv_last"]
    assert close(e["sums"], np.stack([gp.sum(0), (gp * xh).sum(0)]))


def test_mask_tensors_are_followed_and_none_means_the_signs_of_h_and_d1():
    n, H, W = 17, 3, 5
    o = R.operands((n, H, W), "float")
    args = (o["q"], o["target"], o["d1"], o["h"])
    rest = (o["z"], o["mean"], o["inv"], o["W1"], o["W2b"], o["norm"])
    none = R.dense_bwd(*args, None, None, *rest)
    same = R.dense_bwd(*args, o["h"], o["d1"], *rest)
    other = R.dense_bwd(*args, o["h_mask"], o["d1_mask"], *rest)
    for k in ("dpre1", "g", "dW1", "small", "gsums"):
        assert np.array_equal(none[k], same[k]), k
        assert not np.array_equal(none[k], other[k]), k
    dp2 = 2.0 * (o["q"] - o["target"]) * o["norm"] * (1.0 - o["q"] ** 2)
    for s in range(n):
        for k in range(R.C):
            want = float(dp2[s] @ o["W2b"][k]) if o["d1_mask"][s, k] > 0 else 0.0
            assert abs(other["dpre1"][s, k] - want) <= REL * np.abs(dp2).max()
    # dW1 has a row for EVERY pixel, the last one of an odd HW included, and it is h's column times dpre1
    assert other["dW1"].shape == (H * W, R.C)
    last = sum(o["h"][s, H * W - 1] * other["dpre1"][s] for s in range(n))
    assert np.abs(last).max() > 0 and close(other["dW1"][H * W - 1], last)


def test_quad_byte_mask_convention_by_hand():
    """k_bn_apply: one byte per quad of channels, bit k of byte q set when channel 4 q + k passed its ReLU"""
    m = np.zeros((2, 32), dtype=np.uint8)
    m[0, 0] = 0b0101                      # row 0: channels 0 and 2
    m[0, 31] = 0b1000                     # row 0: channel 127
    m[1, 1] = 0b0010                      # row 1: channel 5
    m[1, 2] = 0b1111                      # row 1: channels 8..11
    m[1, 3] = 0xF0                        # the four high bits mean nothing
    bits = R.unpack_quad_bits(m)
    assert sorted(np.flatnonzero(bits[0])) == [0, 2, 127] and sorted(np.flatnonzero(bits[1])) == [5, 8, 9, 10, 11]
    assert np.array_equal(R.pack_quad_bits(bits)[:, :3], m[:, :3]) and R.pack_quad_bits(bits)[1, 3] == 0
    # through conv1x1_bwd: dz = 1 in both rows (A = 1, B = C = 0), w = channel number + 1 -> g' = w where the bit is set
    w = np.arange(1.0, 129.0)
    e = R.conv1x1_bwd(np.ones(2), np.zeros(2), 0.0, 1.0, (1.0, 0.0, 0.0), np.ones((2, 128)), w, np.full((2, 128), 3.0), m,
                      np.ones(128), np.full(128, 0.5))
    want = np.zeros(128)
    for ch in (0, 2, 127, 5, 8, 9, 10, 11):
        want[ch] = ch + 1.0
    assert np.array_equal(e["sums"][0], want) and np.array_equal(e["sums"][1], want * (3.0 - 1.0) * 0.5)
    assert np.array_equal(e["dw1x1"], np.full(128, 2.0)) and np.array_equal(e["da"], np.stack([w, w]))


def test_cases_meet_the_entry_points_limits_and_cover_the_edges():
    ns, canvases = {c[0] for c in R.CASES}, {c[1:] for c in R.CASES}
    assert ns == {1, 2, 15, 16, 17, 33}
    assert canvases == {(3, 5), (1, 5), (4, 6), (13, 13), (21, 13), (21, 21), (37, 37)}
    assert len(set(R.CASES)) == len(R.CASES) <= 16
    for n, H, W in R.CASES:
        assert R.STATES_PER_BLOCK * (H * W + 128) * 4 <= R.LDS_LIMIT              # the forward's LDS
        assert n <= 33 and n * H * W * 128 * 4 <= 12 * 2 ** 20                    # tensors of at most 12 MB
    for hw in canvases:
        assert any(c[1:] == hw and c[0] % 16 for c in R.CASES) and any(c[1:] == hw and c[0] >= 17 for c in R.CASES), hw
    assert any(n == 1 and (H * W) % 2 for n, H, W in R.CASES)
    assert R.CASES.count((17, 37, 37)) == 1 and sum(c[1:] == (37, 37) and c[0] > 2 for c in R.CASES) == 1
    assert R.STATES_PER_BLOCK * (49 * 49 + 128) * 4 > R.LDS_LIMIT                 # the canvas the GPU test expects to be refused
    # the row grid: more than one sweep only for the largest case; folds of fewer than 32 groups and of more
    over = [c for c in R.CASES if c[0] * c[1] * c[2] > R.ROW_BLOCKS * R.ROWS_PER_SWEEP]
    assert over == [(17, 37, 37)] and R.rows_per_block(17 * 37 * 37) == 16 and R.rows_per_block(33 * 21 * 21) == 8
    groups = [R.row_blocks(n * H * W) for n, H, W in R.CASES]
    assert min(groups) < 32 < max(groups) == 2048


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: "%dx%dx%d" % c)
def test_integer_cases_keep_every_partial_sum_below_2_to_the_24(case):
    """so that the GPU test's `bit for bit` rests on arithmetic done here and not on the kernel: operands that are whole numbers of
    a power-of-two quantum, and the absolute values of all terms one float32 accumulation can meet add up to less than 2^24 quanta"""
    head = R.int_headroom(case)
    assert set(head) == {"z", "sums", "h", "d1", "dp2", "dpre1", "g", "dW1", "small", "gsums", "da", "dw1x1", "stat_sums"}
    for name, (s_max, whole) in head.items():
        assert whole, name
        assert 0 < s_max < 2.0 ** 24, (name, s_max)
    o = R.operands(case, "int")
    for k, v in o.items():                                                       # every operand is a float32 as it stands
        if isinstance(v, np.ndarray) and v.dtype == np.float64:
            assert np.array_equal(v.astype(np.float32).astype(np.float64), v), k
    q4 = o["q"] * 4
    assert np.array_equal(q4, np.round(q4)) and np.abs(o["q"]).max() < 1


def test_a_dropped_term_exceeds_the_bound_at_the_largest_term_count():
    """(K + 8) 2^-24 S against one term of typical size S / K: the bound is below it while K (K + 8) < 2^24, i.e. up to K = 4091;
    the largest K of CASES is 1369 (the Dense(128) reduction over 37 x 37 pixels), 21 904 for the two sums over a block of 16 such
    states, where the test leans on the integer cases instead"""
    K = max(H * W for _, H, W in R.CASES)
    assert K == 1369 and R.bound(K, 1.0) < 1.0 / K and K * (K + 8) < 2 ** 24
    o = R.operands((2, 37, 37), "float")
    f = R.dense_fwd(o["z"], o["scale"], o["shift"], o["W1"], o["b1"], o["W2"], o["b2"], o["target"], o["err_scale"])
    h = f["h"].copy()
    px = int(np.flatnonzero((h > 0).all(0))[-1])                                 # the last pixel that is live in both states:
    h[:, px] = 0.0                                                               # its term dropped from every dot product
    wrong = h @ o["W1"] + o["b1"]
    live = np.abs(f["h"][:, px:px + 1] * o["W1"][px]) > 0
    miss = np.abs(wrong - f["pre1"]) > R.bound(K, f["S_pre1"])
    assert live.sum() > 100 and miss[live].mean() > 0.9                          # (terms far below the typical size can hide)
    # and the reference's own float32 evaluation, in another order, stays inside it
    z32 = np.maximum(o["z"].astype(np.float32) * np.float32(o["scale"]) + np.float32(o["shift"]), np.float32(0))
    acc = np.zeros((2, R.C), dtype=np.float32)
    for i in range(K - 1, -1, -1):
        acc += z32[:, i:i + 1] * o["W1"][i].astype(np.float32)
    acc += o["b1"].astype(np.float32)
    err = np.abs(acc.astype(np.float64) - f["pre1"]) / R.bound(K, f["S_pre1"])
    assert err.max() < 1.0
