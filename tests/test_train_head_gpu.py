"""The training head's five kernels (csrc/train_net.hip: k_head1x1, k_head_dense_train_fwd, k_head_dense_train_bwd, k_head_dw1,
k_head_expand<false / true>) one entry point at a time against the float64 definitions of tests/train_head_ref.py, at the shapes
of its CASES: short last blocks of 16 states, one state, odd HW, HW below 8 / no multiple of 8 / below and above 256 threads,
rectangular canvases, more rows than one sweep of the row grid, folds of fewer and of more than 32 groups.

Every output and every input lives inside an allocation filled with NaN: after a launch the output proper is finite and what lies
in front of it and behind it is still NaN (a write to pixel row HW of dW1, to state n of a short block), and a read outside an
input shows as a NaN in a result.  Partial buffers have exactly the advertised sizes.

Two kinds of operand (train_head_ref.operands):
  int    small whole numbers and powers of two; every partial sum is an exact float32 (tests/test_train_head_ref_cpu.py proves the
         headroom), so every output but q and the squared error equals the float64 value's float32 rounding EXACTLY (the sign of a
         zero aside), whatever the order of summation.  One dropped, doubled or misplaced term changes a whole number.
  float  O(1) random values; every element within (K + 8) 2^-24 S of the float64 value, K = the terms of its dot product (per
         block for two-stage sums, the fold being float64), S = the float64 sum of the absolute values of the terms.  A later stage's
         reference starts from the kernel's own, already checked, output of the stage before (d1 for q, q for the squared error,
         dpre1 for g / dW1 / db1, g and da for the sums), so each stage is held to its own bound.  q: the bound of tanh's argument
         (slope <= 1) plus 2^-21 for tanhf.

Largest error as a fraction of its bound over the float cases, one MI355X run (how much slack the rigorous bound leaves):
  snk_head_conv1x1_sums      z 0.0093   sums 0.066
  snk_head_dense_train_fwd   h 0.19   d1 0.20   q 0.010 (2^-21 included)   squared error 0.068
  snk_head_dense_train_bwd   dpre1 0.30   g 0.031   dW1 0.18   small 0.10   the two float64 sums 0.067
  snk_head_conv1x1_bwd       da 0.36   dw1x1 0.097   the 256 sums of the _stats form 0.11
(each test prints its own as `FRACTION <entry point> <case> <output> <value>`; run with -s to see them)
"""
import functools

import numpy as np
import pytest

import train_head_ref as R

pytestmark = pytest.mark.gpu

PAD = 64                                         # canary elements on either side (256 bytes of float32: float4 loads stay aligned)
CASE_IDS = ["%dx%dx%d" % c for c in R.CASES]
KINDS = ["int", "float"]
TANHF = 2.0 ** -21


@pytest.fixture(scope="module")
def gpu():
    import torch
    from snake_engine._lib import lib, check
    assert torch.cuda.is_available()
    return torch, lib(), check, torch.cuda.current_stream().cuda_stream


@functools.lru_cache(maxsize=8)
def operands(case, kind):
    return R.operands(case, kind)


class Guarded:
    """`numel` elements with PAD canaries on either side, all NaN (bytes: 0xFF) until written"""

    def __init__(self, torch, numel, dtype=None, fill=None):
        dtype = dtype or torch.float32
        self.byte = dtype == torch.uint8
        self.full = torch.full((PAD + numel + PAD,), 0xFF if self.byte else float("nan"), dtype=dtype, device="cuda")
        self.body = self.full[PAD:PAD + numel]
        if fill is not None:
            self.body.copy_(torch.as_tensor(np.ascontiguousarray(fill).reshape(-1)).to(dtype))
        self.ptr = self.body.data_ptr()

    def canaries_intact(self):
        edge = self.full[:PAD], self.full[PAD + self.body.numel():]
        return all(bool((e == 0xFF).all()) if self.byte else bool(e.isnan().all()) for e in edge)

    def written(self):
        """the output proper, as float64, after checking that all of it was written and nothing around it"""
        assert self.canaries_intact(), "a write outside the output"
        assert bool(self.body.isfinite().all()), "part of the output was not written (or a NaN from outside an input was read)"
        return self.body.double().cpu().numpy()

    def untouched(self):
        return bool(self.full.isnan().all())


def hold(tag, got, ref, K, S, kind, extra=0.0, exact_in_float32=True):
    """int: got equals the reference (rounded to float32 where the output is one); float: every element within its own bound"""
    ref = R.f64(ref).reshape(got.shape)
    if kind == "int":
        want = ref.astype(np.float32).astype(np.float64) if exact_in_float32 else ref
        bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
        assert bad.size == 0, (tag, bad[:8], got.reshape(-1)[bad[:8]], want.reshape(-1)[bad[:8]])
        return
    lim = R.bound(K, R.f64(S).reshape(got.shape)) + extra
    err = np.abs(got - ref)
    frac = float((err / np.where(lim > 0, lim, 1.0))[lim > 0].max()) if (lim > 0).any() else 0.0
    print("FRACTION %s %.3g" % (tag, frac))
    bad = np.flatnonzero((err > lim).reshape(-1))
    assert bad.size == 0, (tag, frac, bad[:8], got.reshape(-1)[bad[:8]], ref.reshape(-1)[bad[:8]])
    assert float(np.abs(ref).max()) > 0, tag


def ins(torch, o, *names):
    return [Guarded(torch, np.size(o[k]), torch.uint8 if k == "mask_last" else None, fill=o[k]) for k in names]


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", R.CASES, ids=CASE_IDS)
def test_conv1x1_and_its_two_sums(gpu, case, kind):
    torch, L, check, st = gpu
    n, H, W = case
    rows, o = n * H * W, operands(case, kind)
    a, w = ins(torch, o, "a", "w1x1")
    cen = Guarded(torch, 1, fill=[o["center"]])
    for center in (None, o["center"]):
        z, part, sums = Guarded(torch, rows), Guarded(torch, L.snk_bn_train_partials()), Guarded(torch, 2, torch.float64)
        check(L.snk_head_conv1x1_sums(a.ptr, w.ptr, rows, cen.ptr if center is not None else None, z.ptr, part.ptr, sums.ptr, st))
        torch.cuda.synchronize()
        assert part.canaries_intact()
        zg, sg = z.written(), sums.written()
        tag = "conv1x1_sums %s center=%s " % (case, center)
        ref = R.conv1x1_sums(o["a"], o["w1x1"], center, z_in=zg)
        hold(tag + "z", zg, ref["z"], R.C, ref["S_z"], kind)
        hold(tag + "sums", sg, ref["sums"], R.rows_per_block(rows), ref["S_sums"], kind, exact_in_float32=False)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", R.CASES, ids=CASE_IDS)
def test_dense_forward(gpu, case, kind):
    torch, L, check, st = gpu
    n, H, W = case
    HW, o = H * W, operands(case, kind)
    z, W1, b1, W2, b2, target = ins(torch, o, "z", "W1", "b1", "W2", "b2", "target")
    ss = Guarded(torch, 2, fill=[o["scale"], o["shift"]])

    def run(with_h_d1, with_error):
        h, d1, q = Guarded(torch, n * HW), Guarded(torch, n * R.C), Guarded(torch, n * 3)
        part, err = Guarded(torch, L.snk_bn_train_partials()), Guarded(torch, 1)
        check(L.snk_head_dense_train_fwd(z.ptr, ss.ptr, W1.ptr, b1.ptr, W2.ptr, b2.ptr, target.ptr if with_error else None,
                                         h.ptr if with_h_d1 else None, d1.ptr if with_h_d1 else None, q.ptr,
                                         part.ptr if with_error else None, err.ptr if with_error else None, o["err_scale"], n, H, W, st))
        torch.cuda.synchronize()
        assert part.canaries_intact()
        assert with_h_d1 or (h.untouched() and d1.untouched())
        assert with_error or (part.untouched() and err.untouched())
        return h, d1, q, err

    h, d1, q, err = run(True, True)
    hg, d1g, qg, eg = h.written().reshape(n, HW), d1.written().reshape(n, R.C), q.written().reshape(n, 3), err.written()
    ref = R.dense_fwd(o["z"], o["scale"], o["shift"], o["W1"], o["b1"], o["W2"], o["b2"], o["target"], o["err_scale"], d1_in=d1g, q_in=qg)
    tag = "dense_fwd %s " % (case,)
    hold(tag + "h", hg, ref["h"], 1, ref["S_h"], kind)
    hold(tag + "d1", d1g, ref["d1"], HW, ref["S_pre1"], kind)
    hold(tag + "q", qg, ref["q"], R.C, ref["S_arg"], "float", extra=TANHF)
    hold(tag + "sq_err", eg, [ref["sq_err"]], 3 * R.STATES_PER_BLOCK, [ref["S_sq_err"]], "float")
    # the ReLUs: exactly zero below the bound, positive above it
    for got, pre, lim in ((hg, ref["pre_h"], R.bound(1, ref["S_h"])), (d1g, ref["pre1"], R.bound(HW, ref["S_pre1"]))):
        assert (got[pre < -lim] == 0).all() and (got[pre > lim] > 0).all() and (got >= 0).all()
        assert (pre < -lim).any() and (pre > lim).any()
    # the optional outputs change nothing else
    _, _, q2, err2 = run(False, True)
    assert torch.equal(q2.body, q.body) and torch.equal(err2.body, err.body) and q2.canaries_intact() and err2.canaries_intact()
    h3, d13, q3, _ = run(True, False)
    assert torch.equal(q3.body, q.body) and torch.equal(h3.body, h.body) and torch.equal(d13.body, d1.body)
    assert q3.canaries_intact() and h3.canaries_intact() and d13.canaries_intact()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", R.CASES, ids=CASE_IDS)
def test_dense_backward(gpu, case, kind):
    torch, L, check, st = gpu
    n, H, W = case
    HW, o = H * W, operands(case, kind)
    q, target, h, d1, z, W1, W2 = ins(torch, o, "q", "target", "h", "d1", "z", "W1", "W2b")
    mi = Guarded(torch, 2, fill=[o["mean"], o["inv"]])
    assert 0.25 < (o["h"] == 0).mean() < 0.75 and 0.25 < (o["d1"] == 0).mean() < 0.75        # about half zeros, like ReLU outputs
    assert ((o["h_mask"] > 0) != (o["h"] > 0)).any() and ((o["d1_mask"] > 0) != (o["d1"] > 0)).any()

    def run(h_mask, d1_mask):
        outs = dict(dpre1=Guarded(torch, n * R.C), g=Guarded(torch, n * HW), dW1=Guarded(torch, HW * R.C), small=Guarded(torch, 515),
                    gsums=Guarded(torch, 2, torch.float64))
        part = Guarded(torch, L.snk_head_dense_train_bwd_partials(n))
        check(L.snk_head_dense_train_bwd(q.ptr, target.ptr, h.ptr, d1.ptr, h_mask.ptr if h_mask else None, d1_mask.ptr if d1_mask else None,
                                         z.ptr, mi.ptr, W1.ptr, W2.ptr, o["norm"], outs["dpre1"].ptr, outs["g"].ptr, outs["dW1"].ptr,
                                         outs["small"].ptr, outs["gsums"].ptr, part.ptr, n, H, W, st))
        torch.cuda.synchronize()
        assert part.canaries_intact()
        return outs, {k: v.written() for k, v in outs.items()}

    def judge(tag, got, h_mask, d1_mask):
        dp, gg = got["dpre1"].reshape(n, R.C), got["g"].reshape(n, HW)
        ref = R.dense_bwd(o["q"], o["target"], o["d1"], o["h"], h_mask, d1_mask, o["z"], o["mean"], o["inv"], o["W1"], o["W2b"], o["norm"],
                          dpre1_in=dp, g_in=gg)
        hold(tag + "dpre1", dp, ref["dpre1"], 3, ref["S_dpre1"], kind)
        hold(tag + "g", gg, ref["g"], R.C, ref["S_g"], kind)
        hold(tag + "dW1", got["dW1"].reshape(HW, R.C), ref["dW1"], n, ref["S_dW1"], kind)
        hold(tag + "small", got["small"], ref["small"], R.STATES_PER_BLOCK, ref["S_small"], kind)
        hold(tag + "gsums", got["gsums"], ref["gsums"], min(n, R.STATES_PER_BLOCK) * HW, ref["S_gsums"], kind, exact_in_float32=False)
        return ref

    none, got_none = run(None, None)
    ref_none = judge("dense_bwd %s masks=NULL " % (case,), got_none, None, None)
    hm, dm = ins(torch, o, "h_mask", "d1_mask")
    _, got_other = run(hm, dm)
    ref_other = judge("dense_bwd %s masks=other " % (case,), got_other, o["h_mask"], o["d1_mask"])
    assert not np.array_equal(ref_none["dpre1"], ref_other["dpre1"]) and not np.array_equal(ref_none["g"], ref_other["g"])
    hs, ds = ins(torch, o, "h", "d1")                    # mask tensors of their own with the signs of h / d1: the bits of the NULL call
    same, _ = run(hs, ds)
    for k in none:
        assert torch.equal(same[k].body, none[k].body), k


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", R.CASES, ids=CASE_IDS)
def test_conv1x1_backward_and_the_last_layers_sums(gpu, case, kind):
    torch, L, check, st = gpu
    n, H, W = case
    rows, o = n * H * W, operands(case, kind)
    g, z, a, w, y, m, mu, iv = ins(torch, o, "g", "zr", "a_last", "w1x1", "y_last", "mask_last", "mean_last", "inv_last")
    mi, abc = Guarded(torch, 2, fill=[o["mean"], o["inv"]]), Guarded(torch, 3, fill=o["abc"])
    P = L.snk_bn_train_partials()
    da_a, dw_a, part_a = Guarded(torch, rows * R.C), Guarded(torch, R.C), Guarded(torch, P)
    check(L.snk_head_conv1x1_bwd(g.ptr, z.ptr, mi.ptr, abc.ptr, a.ptr, w.ptr, da_a.ptr, dw_a.ptr, part_a.ptr, rows, st))
    da_b, dw_b, part_b, part2, sums = Guarded(torch, rows * R.C), Guarded(torch, R.C), Guarded(torch, P), Guarded(torch, P), \
        Guarded(torch, 2 * R.C, torch.float64)
    check(L.snk_head_conv1x1_bwd_stats(g.ptr, z.ptr, mi.ptr, abc.ptr, a.ptr, w.ptr, da_b.ptr, dw_b.ptr, part_b.ptr, y.ptr, m.ptr, mu.ptr,
                                       iv.ptr, part2.ptr, sums.ptr, rows, st))
    torch.cuda.synchronize()
    assert part_a.canaries_intact() and part_b.canaries_intact() and part2.canaries_intact()
    dag, dwg, sg = da_a.written().reshape(rows, R.C), dw_a.written(), sums.written().reshape(2, R.C)
    da_b.written(), dw_b.written()
    assert torch.equal(da_a.body, da_b.body) and torch.equal(dw_a.body, dw_b.body)
    ref = R.conv1x1_bwd(o["g"], o["zr"], o["mean"], o["inv"], o["abc"], o["a_last"], o["w1x1"], o["y_last"], o["mask_last"],
                        o["mean_last"], o["inv_last"], da_in=dag)
    tag, K = "conv1x1_bwd %s " % (case,), R.rows_per_block(rows)
    hold(tag + "da", dag, ref["da"], 3, ref["S_da"], kind)
    hold(tag + "dw1x1", dwg, ref["dw1x1"], K, ref["S_dw1x1"], kind)
    hold(tag + "stat_sums", sg, ref["sums"], K, ref["S_sums"], kind, exact_in_float32=False)


# ---------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing_and_name_the_function(gpu):
    """n_images = 0 / rows = 0, each required pointer NULL in turn, d_sq_err without d_target (or without d_partials), and for the
    forward a 49 x 49 canvas (16 (2401 + 128) floats = 158 KB of LDS against the kernel's 150 KB): a non-zero return, the function's
    name in snk_last_error(), and every output still NaN"""
    torch, L, check, st = gpu
    n, H, W = 2, 49, 49                                   # buffers large enough for the canvas that is refused; valid calls use 1 x 5
    HW, rows = H * W, n * H * W
    rs = np.random.RandomState(5)
    f = lambda numel, dtype=None: Guarded(torch, numel, dtype, fill=rs.randint(0, 4, size=numel))
    a, w, z, W1, b1, W2, b2, tgt, ss = f(rows * R.C), f(R.C), f(rows), f(HW * R.C), f(R.C), f(R.C * 3), f(3), f(n * 3), f(2)
    qv, hv, d1v, mi, abc, gv, y, mu, iv = f(n * 3), f(rows), f(n * R.C), f(2), f(3), f(rows), f(rows * R.C), f(R.C), f(R.C)
    m = f(rows * 32, torch.uint8)
    outs = []

    def out(numel, dtype=None):
        outs.append(Guarded(torch, numel, dtype))
        return outs[-1].ptr

    P = L.snk_bn_train_partials()
    calls = {
        "snk_head_conv1x1_sums": ([a.ptr, w.ptr, 10, None, out(rows), out(P), out(2, torch.float64), st], [0, 1, 4, 5, 6], [2]),
        "snk_head_dense_train_fwd": ([z.ptr, ss.ptr, W1.ptr, b1.ptr, W2.ptr, b2.ptr, tgt.ptr, out(rows), out(n * R.C), out(n * 3), out(P),
                                      out(1), 0.5, n, 1, 5, st], [0, 1, 2, 3, 4, 5, 9], [13]),
        "snk_head_dense_train_bwd": ([qv.ptr, tgt.ptr, hv.ptr, d1v.ptr, None, None, z.ptr, mi.ptr, W1.ptr, W2.ptr, 0.5, out(n * R.C),
                                      out(rows), out(HW * R.C), out(515), out(2, torch.float64),
                                      out(L.snk_head_dense_train_bwd_partials(n)), n, 1, 5, st], [0, 1, 2, 3, 6, 7, 8, 9, 11, 12, 13, 14, 15, 16], [17]),
        "snk_head_conv1x1_bwd": ([gv.ptr, z.ptr, mi.ptr, abc.ptr, a.ptr, w.ptr, out(rows * R.C), out(R.C), out(P), 10, st],
                                 list(range(9)), [9]),
        "snk_head_conv1x1_bwd_stats": ([gv.ptr, z.ptr, mi.ptr, abc.ptr, a.ptr, w.ptr, out(rows * R.C), out(R.C), out(P), y.ptr, m.ptr, mu.ptr,
                                        iv.ptr, out(P), out(2 * R.C, torch.float64), 10, st], list(range(15)), [15]),
    }
    refused = 0
    for name, (args, pointers, counts) in calls.items():
        variants = [(i, None) for i in pointers] + [(i, 0) for i in counts]
        if name == "snk_head_dense_train_fwd":
            variants += [(6, None), (10, None), ((14, 15), 49)]          # d_sq_err without d_target / without d_partials; 49 x 49
        for where, value in variants:
            bad = list(args)
            for i in (where if isinstance(where, tuple) else (where,)):
                bad[i] = value
            assert getattr(L, name)(*bad) != 0, (name, where)
            msg = L.snk_last_error().decode()
            assert msg.startswith(name + ":"), (name, where, msg)
            refused += 1
    torch.cuda.synchronize()
    assert refused == 5 + 1 + 7 + 1 + 3 + 14 + 1 + 9 + 1 + 15 + 1
    for o_ in outs:
        assert o_.untouched()
    with pytest.raises(Exception, match="snk_head_conv1x1_sums"):
        check(L.snk_head_conv1x1_sums(a.ptr, w.ptr, 0, None, outs[0].ptr, outs[1].ptr, outs[2].ptr, st))
    # and the same argument lists are accepted as they stand: the refusals above were about the one argument changed
    for name, (args, _, _) in calls.items():
        check(getattr(L, name)(*args))
    torch.cuda.synchronize()
    assert all(o_.canaries_intact() for o_ in outs)
