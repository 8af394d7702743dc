"""tests/wgrad_ref.py against what it restates, without a GPU: dw_ref against float64 autograd, the launch table against the boundaries
derived from wg2_shape by hand, the case table of tests/test_wgrad_stream_gpu.py against the launch table, and the two float32
reciprocal divisions of slot_off (csrc/train_wgrad.hip) against integer division up to the size the launcher admits."""
import re

import numpy as np
import pytest

import wgrad_ref


@pytest.mark.parametrize("n,h,w", [(1, 1, 3), (2, 1, 4), (3, 2, 3), (2, 3, 5), (2, 5, 3), (1, 4, 4)])
def test_dw_ref_is_the_gradient_of_a_float64_convolution(n, h, w):
    import torch
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(100 * n + 10 * h + w)
    x = torch.randn(n, h, w, 128, dtype=torch.float64, generator=g)
    dy = torch.randn(n, h, w, 128, dtype=torch.float64, generator=g)
    k = torch.zeros(3, 3, 128, 128, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(x.permute(0, 3, 1, 2), k.permute(3, 2, 0, 1), padding=1)
    want, = torch.autograd.grad(y, (k,), dy.permute(0, 3, 1, 2))
    got = wgrad_ref.dw_ref(x, dy)
    assert got.dtype == torch.float64 and got.shape == (3, 3, 128, 128)
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
    got32 = wgrad_ref.dw_ref(x.float(), dy.float(), torch.float32)
    assert got32.dtype == torch.float32 and float((got32.double() - want).abs().max()) <= 1e-4 * float(want.abs().max())


def test_launch_table_has_the_boundaries_derived_from_the_source():
    c = wgrad_ref.constants()
    assert (c["WG_GROUPS"], c["WG2_GROUPS"], c["NK_MAX"], c["WT"]) == (16, 128, 5, (21, 37))
    for h in (1, 2, 5, 20, 22, 36, 38, 50):                  # no square 21 / 37 among them: the window form never looks at the height
        for w in range(3, 97):
            want = (5, 4, 0) if w <= 22 else (5, 5, 0) if w <= 29 else (4, 4, 0) if w == 30 else (4, 5, 0) if w <= 46 else "slab"
            assert wgrad_ref.body(h, w, c) == want, (h, w)
    assert wgrad_ref.body(21, 21, c) == (5, 4, 21) and wgrad_ref.body(37, 37, c) == (4, 5, 37)
    assert wgrad_ref.body(21, 37, c) == (4, 5, 0) and wgrad_ref.body(37, 21, c) == (5, 4, 0)
    for h, w in ((0, 5), (5, 2), (5, 97)):                   # "width 3 .. 96"
        with pytest.raises(ValueError):
            wgrad_ref.body(h, w, c)


def test_launch_lines_in_the_source_are_the_ones_restated():
    """the WG2_LAUNCH lines of wgrad_launch, in their order: a line added, dropped or re-ordered there must be restated in body()"""
    with open(wgrad_ref.SRC) as f:
        text = f.read()
    lines = re.findall(r"^\s+(?:else )?(?:if \((.*)\) )?WG2_LAUNCH\((\d+), (\d+), (\d+)\)$", text, re.M)
    assert lines == [("wt == 21 && s2.nk == 5 && s2.maxx <= 4", "5", "4", "21"), ("wt == 21 && s2.nk == 4 && s2.maxx <= 4", "4", "4", "21"),
                     ("wt == 37 && s2.nk == 4 && s2.maxx <= 5", "4", "5", "37"), ("s2.nk == 5 && s2.maxx <= 4", "5", "4", "0"),
                     ("s2.nk == 5", "5", "5", "0"), ("s2.maxx <= 4", "4", "4", "0"), ("", "4", "5", "0")]


def test_case_table_reaches_every_body_with_the_group_pattern_it_claims():
    c = wgrad_ref.constants()
    reachable = {wgrad_ref.body(h, w, c) for h in range(1, 98) for w in range(3, 97)}
    # six of the seven launch lines ((4, 4, 21) needs SNK_WGRAD_NK=4, a development knob) and the slab form
    assert reachable == {(5, 4, 21), (4, 5, 37), (5, 4, 0), (5, 5, 0), (4, 4, 0), (4, 5, 0), "slab"}
    assert {b for _, _, _, b, _ in wgrad_ref.CASES} == reachable
    for n, h, w, b, pattern in wgrad_ref.CASES:
        assert wgrad_ref.body(h, w, c) == b, (n, h, w)
        g, per, full, short, empty = pattern
        assert g == (16 if b == "slab" else 128) and per == -(-n // g), (n, h, w)
        sizes = [max(0, min(per, n - i * per)) for i in range(g)]             # n0 = grp * per_group, n1 = min(n0 + per_group, n)
        assert sum(sizes) == n
        assert (sizes.count(per), sum(s for s in sizes if 0 < s < per), sizes.count(0)) == (full, short, empty), (n, h, w)
        assert sum(1 for s in sizes if 0 < s < per) == (1 if short else 0)
        assert wgrad_ref.groups(n, h, w, c=c) == pattern
        assert per >= 2, "every case is there for more than one image in a group"
    for n, h, w, pattern in wgrad_ref.SLAB_SWITCH:
        assert wgrad_ref.body(h, w, c) != "slab" and wgrad_ref.groups(n, h, w, slabs=True, c=c) == pattern and pattern[1] >= 2
    # what the table is there for, each met by at least one window case
    win = [(n, h, w, p) for n, h, w, b, p in wgrad_ref.CASES if b != "slab"]
    assert any(p[3] for _, _, _, p in win) and any(p[3] == 0 for _, _, _, p in win)      # a shorter last group; none
    assert any(h > w for _, h, w, _ in win) and any(h < w for _, h, w, _ in win) and any(h == 1 for _, h, w, _ in win)
    for n, h, w, p in win:                                                   # a window that starts in one image and ends in the next
        nk = wgrad_ref.wg2_shape(h, w, c)[0]
        assert (h + 1) * (w + 1) % (16 * nk) != 0, (n, h, w)


def _div_model(s, d):
    """slot_off's division: (int)(((float)s + 0.5f) * (1.0f / d)), every operation rounded to float32"""
    inv = np.float32(1.0) / np.float32(d)
    return ((s.astype(np.float32) + np.float32(0.5)) * inv).astype(np.int32)


def test_the_reciprocal_divisions_of_slot_off_are_exact_below_the_launcher_bound():
    """the launcher admits per_group (H + 1) (W + 1) < 2^22 slots; r = s / P and i = r / SR are taken as float32 products with a
    reciprocal.  Every P = W + 1 of the widths 3 .. 96 and every SR = H + 1 from 2 (H = 1) to 97, every s below 2^22 (a stream row r
    is below it as well); larger SR at the values around its powers of two and its largest, 2^20 (W = 3)."""
    with open(wgrad_ref.SRC) as f:
        text = f.read()
    assert "const int r = (int)(((float)s + 0.5f) * invP)" in text and "const int i = (int)(((float)r + 0.5f) * invSR)" in text
    assert "const float invP = 1.0f / (float)P, invSR = 1.0f / (float)SR;" in text
    assert "(long)per_group * (height + 1) * (width + 1) < (1l << 22)" in text
    s = np.arange(1 << 22, dtype=np.int32)
    for d in range(2, 98):
        bad = np.flatnonzero(_div_model(s, d) != s // d)
        assert bad.size == 0, (d, bad[:5])
    r = np.arange(1 << 20, dtype=np.int32)                   # stream rows: s / P with P >= 4
    for k in range(7, 21):
        for d in ((1 << k) - 1, 1 << k, (1 << k) + 1, 3 << (k - 1)):
            bad = np.flatnonzero(_div_model(r, d) != r // d)
            assert bad.size == 0, (d, bad[:5])
