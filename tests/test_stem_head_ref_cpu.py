"""tests/stem_head_ref.py, the float64 model tests/test_stem_forms_gpu.py and tests/test_head_forms_gpu.py hold the inference stem
and head to, proven without a GPU: the stem against float64 torch conv2d, the box decoding against cases written out by hand, the
two head functions against each other and (stem -> head, no tower) against oracle/net_ref.py on golden states; and the one piece of
kernel arithmetic that is not obviously exact, the MFMA stem's float32 row index, restated and swept over its whole domain."""
import numpy as np
import pytest

import stem_head_ref as R
from conftest import load_golden

REL = 1e-12


@pytest.mark.parametrize("n,H,W", [(2, 1, 1), (1, 1, 5), (3, 4, 7), (2, 9, 9)])
def test_stem_equals_float64_conv2d(n, H, W):
    import torch
    rs = np.random.RandomState(100 * H + W)
    x = rs.rand(n, H, W, 3) * 6 - 1
    w = rs.randn(3, 3, 3, R.C) * 0.2
    scale, shift = rs.rand(R.C) + 0.5, rs.randn(R.C) * 0.1
    conv = torch.nn.functional.conv2d(torch.tensor(x).permute(0, 3, 1, 2), torch.tensor(w).permute(3, 2, 0, 1), padding=1)
    conv = conv.permute(0, 2, 3, 1).numpy()
    raw = R.stem(x, w, None, None, raw=True)
    assert raw.dtype == np.float64 and raw.shape == (n, H, W, R.C)
    assert np.abs(raw - conv).max() <= REL * np.abs(conv).max()
    want = np.maximum(conv * scale + shift, 0.0)
    got = R.stem(x, w, scale, shift)
    assert np.abs(got - want).max() <= REL * np.abs(want).max()
    assert (got == 0).any() and (got > 0).any()             # the ReLU clamps some and passes some


def test_pack_bbox_layout():
    assert R.pack_bbox(1, 2, 3, 4) == 0x04030201
    b = R.pack_bbox(1, 150, 2, 199)
    assert b.dtype == np.uint32 and int(b) == 1 | 150 << 8 | 2 << 16 | 199 << 24 and int(b) >> 31 == 1
    assert int(np.array([b], dtype=np.uint32).view(np.int32)[0]) < 0          # as the int32 the caller's array holds: negative


def test_rect_mask_hand_written_cases():
    # a corner box: rows 0..0, columns 0..0 grown by 1 on a 5 x 6 canvas -> rows 0..1, columns 0..1
    m = R.rect_mask([R.pack_bbox(0, 0, 0, 0)], 1, 5, 6)
    want = np.zeros((1, 5, 6), dtype=bool)
    want[0, 0, 0] = want[0, 0, 1] = want[0, 1, 0] = want[0, 1, 1] = True
    assert m.dtype == bool and np.array_equal(m, want)
    # the opposite corner, grow 2: rows 2..4, columns 3..5
    m = R.rect_mask([R.pack_bbox(4, 5, 4, 5)], 2, 5, 6)
    want = np.zeros((1, 5, 6), dtype=bool)
    for y in (2, 3, 4):
        for x in (3, 4, 5):
            want[0, y, x] = True
    assert np.array_equal(m, want)
    # the whole canvas stays the whole canvas
    assert R.rect_mask([R.pack_bbox(0, 0, 4, 5)], 1, 5, 6).all()
    # grow larger than the canvas: any box becomes the whole image
    assert R.rect_mask([R.pack_bbox(2, 3, 2, 3)], 127, 5, 6).all()
    # an inner box keeps its margin: (2,2)-(2,3) grown by 1 on 5 x 6 -> rows 1..3, columns 1..4 = 12 pixels
    m = R.rect_mask([R.pack_bbox(2, 2, 2, 3)], 1, 5, 6)
    assert m.sum() == 12 and m[0, 1:4, 1:5].all()
    # x1 = 199 on a 4 x 200 canvas (bit 31 of the packed box): rows 0..3, columns 149..199
    m = R.rect_mask(np.array([R.pack_bbox(1, 150, 2, 199)], dtype=np.uint32).view(np.int32), 1, 4, 200)
    assert m.sum() == 4 * 51 and m[0, :, 149:].all() and not m[0, :, :149].any()
    # one box per image
    m = R.rect_mask([R.pack_bbox(0, 0, 0, 0), R.pack_bbox(3, 3, 3, 3)], 1, 4, 4)
    assert m.shape == (2, 4, 4) and m[0].sum() == 4 and m[1].sum() == 4 and m[0, :2, :2].all() and m[1, 2:, 2:].all()


def _head_inputs(rs, n, H, W):
    act = rs.randn(n, H, W, R.C)
    return dict(act=act, w1=rs.randn(R.C) * 0.1, s1=0.7, b1=0.05, fc1_w=rs.randn(H * W, R.C) * 0.05, fc1_b=rs.randn(R.C) * 0.1,
                fc2_w=rs.randn(R.C, 3) * 0.1, fc2_b=rs.randn(3) * 0.1)


@pytest.mark.parametrize("n,H,W", [(1, 1, 1), (3, 1, 3), (4, 5, 6)])
def test_head_equals_head_dense_of_its_h1(n, H, W):
    rs = np.random.RandomState(7 * n + H * W)
    d = _head_inputs(rs, n, H, W)
    mask = (rs.rand(n, 3) < 0.4).astype(np.uint8)
    mask[0, 0] = 1
    for m in (None, mask):
        h1, q = R.head(d["act"], d["w1"], d["s1"], d["b1"], d["fc1_w"], d["fc1_b"], d["fc2_w"], d["fc2_b"], m)
        assert h1.shape == (n, H * W) and q.shape == (n, 3) and h1.dtype == np.float64 and (h1 >= 0).all()
        assert np.array_equal(q, R.head_dense(h1, d["fc1_w"], d["fc1_b"], d["fc2_w"], d["fc2_b"], m))
        assert np.array_equal(q, R.head_dense(h1.reshape(n, H, W), d["fc1_w"], d["fc1_b"], d["fc2_w"], d["fc2_b"], m))
        if m is not None:
            assert (q[m != 0] == -1.0).all() and (np.abs(q[m == 0]) < 1.0).all()
    # by hand: one pixel, act = e_0, w1 = 2 e_0 -> z = 2, h1 = max(2 * 0.5 - 0.25, 0) = 0.75
    act = np.zeros((1, 1, 1, R.C))
    act[0, 0, 0, 0] = 1.0
    w1 = np.zeros(R.C)
    w1[0] = 2.0
    fc1_w = np.zeros((1, R.C))
    fc1_w[0, 5] = 2.0                                       # h2 = relu(1.5 e_5 + fc1_b), fc1_b = -0.5 e_5 - e_6 -> e_5
    fc1_b = np.zeros(R.C)
    fc1_b[5], fc1_b[6] = -0.5, -1.0
    fc2_w = np.zeros((R.C, 3))
    fc2_w[5] = (1.0, -2.0, 0.0)
    fc2_w[6] = (100.0, 100.0, 100.0)                        # behind a clamped h2: no effect
    h1, q = R.head(act, w1, 0.5, -0.25, fc1_w, fc1_b, fc2_w, np.array([0.0, 0.0, 0.25]), np.array([[0, 0, 0]]))
    assert h1[0, 0] == 0.75 and np.allclose(q[0], np.tanh([1.0, -2.0, 0.25]), rtol=1e-15, atol=0)


def test_stem_then_head_equals_the_net_oracle_without_a_tower():
    """a 0-block weight list is stem -> head: oracle/net_ref.py (float32 torch, the oracle of the whole net) and this model agree"""
    from oracle import net_ref
    from snake_engine import net
    ws = net.glorot_uniform_weights((21, 21, 3), blocks=0, seed=3)
    assert len(ws) == 14
    rs = np.random.RandomState(0)
    ws[1:5] = [(1 + 0.2 * rs.randn(R.C)).astype(np.float32), (0.1 * rs.randn(R.C)).astype(np.float32),
               (0.05 * rs.randn(R.C)).astype(np.float32), (0.5 + rs.rand(R.C)).astype(np.float32)]
    ws[6:10] = [np.float32([1.3]), np.float32([-0.05]), np.float32([0.02]), np.float32([0.8])]
    ws[11] = (0.1 * rs.randn(R.C)).astype(np.float32)
    ws[13] = (0.1 * rs.randn(3)).astype(np.float32)
    states = load_golden("states_11x11x4.npz")["raw"][:8]
    assert states.shape == (8, 21, 21, 3)

    def fold(g, b, m, v):
        s = R.f64(g) / np.sqrt(R.f64(v) + net_ref.BN_EPS)
        return s, R.f64(b) - R.f64(m) * s
    sc, sh = fold(*ws[1:5])
    a = R.stem(states, ws[0], sc, sh)
    # the 1x1 stage's running mean = the median of its pre-activation: half of h1 is clamped, half passes
    ws[8] = np.float32([np.median(a.reshape(-1, R.C) @ R.f64(ws[5]).reshape(R.C))])
    want = net_ref.forward(ws, states, apply_mask=False)
    s1, b1 = fold(*ws[6:10])
    h1, q = R.head(a, ws[5].reshape(R.C), s1[0], b1[0], ws[10], ws[11], ws[12], ws[13])
    assert 0.3 < (h1 > 0).mean() < 0.7 and np.abs(q).max() > 1e-3
    assert np.abs(q - want).max() <= 1e-6, np.abs(q - want).max()


def test_launcher_model_reaches_the_forms_the_gpu_cases_name():
    # the group size of k_stem_conv_mfma for the full-canvas cases of tests/helpers/stem_forms_runner.py
    assert [R.stem_group(n, H, W) for n, H, W in ((7, 35, 35), (5, 38, 38), (3, 45, 45), (2, 55, 55), (1, 71, 71), (2051, 5, 7))] \
        == [3, 3, 2, 1, 1, 4]
    assert R.stem_lds_bytes(71, 71) == 63948 and R.stem_lds_bytes(72, 72) == 65712 and R.stem_lds_bytes(3, 1200) > R.LDS_64K
    assert (2051 + 3) // 4 == 513 and 2051 - 512 * 4 == 3            # 513 groups on 512 blocks, the last one of 3 images
    # k_head_dense's template argument for the canvases of tests/test_head_forms_gpu.py
    assert [R.head_dense_states_per_block(H, W) for H, W in ((1, 5), (21, 21), (20, 20), (37, 37), (45, 45), (62, 64), (63, 63))] \
        == [16, 16, 16, 8, 4, 4, 0]
    assert 4 * (62 * 64 + 128) * 4 == R.LDS_64K


def test_float32_row_index_is_exact_on_every_canvas_that_fits_64k():
    """k_stem_conv_mfma finds a pixel's row without an integer division: yr = int((float(pix) + 0.5f) * (1.0f / float(wr))).
    It equals pix // wr for every rectangle width wr and every pixel number of the tallest canvas of that width whose padded copy
    fits 64 KB of LDS, (H + 2)(wr + 2) <= 5461 -- a sub-rectangle is never wider or taller than its canvas.  Whoever widens the
    LDS budget has to widen this sweep with it."""
    cells = R.LDS_64K // 12
    assert cells == 5461
    checked = 0
    for wr in range(1, 1819):
        H = cells // (wr + 2) - 2
        assert H >= 1
        pix = np.arange(H * wr, dtype=np.int64)
        got = R.row_index_f32(pix, wr)
        bad = np.nonzero(got != pix // wr)[0]
        assert bad.size == 0, (wr, int(pix[bad[0]]), int(got[bad[0]]))
        checked += pix.size
    assert cells // (1819 + 2) - 2 < 1                               # no wider canvas has a row
    assert checked > 5_000_000
