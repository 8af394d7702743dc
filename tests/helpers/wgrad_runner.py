"""The case runner of tests/test_wgrad_stream_gpu.py: operands, guarded buffers and the launch of one weight-gradient entry point.

Imported by that test; run as a program it is the test's child process under SNK_WGRAD=slabs (the switch is read once per process):
the exact-integer check of the split entry for the shapes of wgrad_ref.SLAB_SWITCH in the slab form, one "ok" line per shape."""
import os
import sys

TESTS = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPO = os.path.dirname(TESTS)
for _p in (TESTS, REPO, os.path.join(REPO, "alphasnake-zero_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import torch

import wgrad_ref

SLACK = 64 * 128                 # floats of NaN in front of and behind every operand
NAN = float("nan")


def guarded(t):
    """a copy of t inside a larger allocation that holds NaN in front of and behind it: a read outside the tensor shows in the result"""
    buf = torch.full((t.numel() + 2 * SLACK,), NAN, dtype=t.dtype, device=t.device)
    v = buf[SLACK:SLACK + t.numel()].view(t.shape)
    v.copy_(t)
    return v


def tail_of(L, x):
    """{., ., scale, 1 / scale} of a tensor, as the element-wise kernels leave it for the convolution that reads it"""
    from snake_engine.net import F16S_TAIL_OFFSET, F16S_WEIGHT_BYTES
    from snake_engine._lib import check
    image = torch.empty(F16S_WEIGHT_BYTES, dtype=torch.uint8, device="cuda")
    part = torch.empty(L.snk_bn_train_partials(), device="cuda")
    check(L.snk_conv3x3_f16s_input_scale(x.data_ptr(), x.numel(), image.data_ptr(), part.data_ptr(), torch.cuda.current_stream().cuda_stream))
    return image[F16S_TAIL_OFFSET:F16S_TAIL_OFFSET + 16].view(torch.float32).clone()


def integers(n, h, w, seed):
    """[n, h, w, 128] of integers in -3 .. 3 drawn per element, one element forced to 3: the tensor's scale is 2^10"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    t = torch.randint(-3, 4, (n, h, w, 128), device="cuda", generator=g).float()
    t.view(-1)[seed % t.numel()] = 3.0 if seed & 1 else -3.0
    return guarded(t)


def channel_transform():
    """scale (1, -1 or 2) and shift (0, 1 or 2, three of four positive) per channel: relu(y * scale + shift) of an integer y is an
    integer, and a padding slot that went through it would become the shift"""
    c = torch.arange(128, device="cuda")
    scale = torch.tensor([-1.0, 1.0, 2.0], device="cuda")[c % 3].contiguous()
    shift = torch.where(c % 4 == 0, 0.0, 1.0 + (c % 2).float()).contiguous()
    return scale, shift


def launch(L, entry, x, dy, tx, tdy, n, h, w, scale=None, shift=None):
    """dw of one entry point (scale / shift: the deferred ones, x is then y_below); partials and dw hold NaN before the launch -- a
    group without images must still write its zeros.  Raises EngineError with the library's message where the call is refused."""
    from snake_engine._lib import check
    st = torch.cuda.current_stream().cuda_stream
    need = L.snk_conv3x3_wgrad_partials(h, w)
    assert need > 0
    part = torch.full((need,), NAN, device="cuda")
    dw = torch.full((3, 3, 128, 128), NAN, device="cuda")
    fn = getattr(L, entry)
    if scale is None:
        check(fn(x.data_ptr(), dy.data_ptr(), tx.data_ptr(), tdy.data_ptr(), part.data_ptr(), dw.data_ptr(), n, h, w, st))
    else:
        check(fn(x.data_ptr(), scale.data_ptr(), shift.data_ptr(), dy.data_ptr(), tx.data_ptr(), tdy.data_ptr(), part.data_ptr(),
                 dw.data_ptr(), n, h, w, st))
    torch.cuda.synchronize()
    return dw


def exact_case(L, n, h, w):
    """integer operands of a case, their scale tails, the float64 gradient, and the precondition of bit-exactness: the sum of
    |x| |dy| behind every output entry is below 2^24, so every float32 partial sum is an exact integer (times 2^20)"""
    x, dy = integers(n, h, w, 2 * n + 1), integers(n, h, w, 2 * n + 2)
    tx, tdy = tail_of(L, x), tail_of(L, dy)
    assert float(tx[2]) == 1024.0 and float(tdy[2]) == 1024.0 and float(tx[3]) == 2.0 ** -10 and float(tdy[3]) == 2.0 ** -10
    ref = wgrad_ref.dw_ref(x, dy)
    assert float(wgrad_ref.dw_ref(x.abs(), dy.abs()).max()) < 2.0 ** 24
    return dict(x=x, dy=dy, tx=tx, tdy=tdy, ref=ref)


def main():
    from snake_engine._lib import lib
    assert os.environ.get("SNK_WGRAD") == "slabs"
    L = lib()
    for n, h, w, pattern in wgrad_ref.SLAB_SWITCH:
        assert L.snk_train_deferred_bn_supported(h, w) == 0, "SNK_WGRAD=slabs: the slab form runs, which has no deferred input"
        c = exact_case(L, n, h, w)
        dw = launch(L, "snk_conv3x3_wgrad_f16s", c["x"], c["dy"], c["tx"], c["tdy"], n, h, w)
        assert torch.equal(dw.double(), c["ref"]), f"{n} x {h} x {w}: {int((dw.double() != c['ref']).sum())} entries differ"
        assert float(c["ref"].abs().max()) > 0
        print(f"ok {n} x {h} x {w} slab form, groups {pattern}")
    print(f"wgrad slabs: {len(wgrad_ref.SLAB_SWITCH)} cases exact")


if __name__ == "__main__":
    main()
