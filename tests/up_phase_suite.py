"""Checks of the up-sampling phase convs (csrc/k_gemm.h, UP: nearest x2 + 3x3 conv as four 2x2-tap convs over the low-resolution image), shared by the
emulator tests and the GPU tests.  Reference and tolerance are those of ops_suite.check_conv: the un-rounded fp32 F.interpolate + F.conv2d, atol 3e-4
(the bar of the F8 3x3 kernel on the same layers).  The engine takes the phase path by launch size (at least two 256-row tiles per CU): the
op-level checks force it at their small shapes with the option conv_up_phase = 2."""
import math

import torch
import torch.nn.functional as F

import ops_suite as S

# N, H, W, Cin, Cout
SHAPES = [
    (2, 5, 7, 64, 128),        # odd sizes, two chunks, tap shifts at the image boundary of a batch, one ragged row tile per image (at the 256 / 128 tile)
    (1, 16, 24, 128, 160),     # ragged output-channel tile, several row tiles
    (2, 9, 33, 32, 256),       # two output-channel tiles, all four phases in each
]


def check_case(eng, dev, shape, seed, counter=True):
    """counter: the caller has set conv_up_phase = 2, and the launch counters must show the phase path and nothing else"""
    N, H, W, Cin, Cout = shape
    eng.lib.kernel_counts(reset=True)
    err = S.check_conv(eng, dev, N, H, W, Cin, Cout, up=1, in_f32=True, out_f32=True, split=True, f8=True, seed=seed, atol=3e-4)
    counts = eng.lib.kernel_counts()
    if counter:
        assert counts.get("conv_up_phase", 0) == 1 and counts.get("conv3x3_f8", 0) == 0, counts
    return err, counts


def check_option_off(eng, dev, set_option):
    """conv_up_phase = 0: the layer keeps no phase matrices and launches what it launched before the phase path existed"""
    set_option(eng, "conv_up_phase", 0)
    off = [check_case(eng, dev, s, 20 + i, counter=False)[1] for i, s in enumerate(SHAPES)]
    for c in off:
        assert c.get("conv_up_phase", 0) == 0, c
    set_option(eng, "conv_up_phase", 1)              # by launch size: these are far too small
    small = [check_case(eng, dev, s, 20 + i, counter=False)[1] for i, s in enumerate(SHAPES)]
    assert small == off, (small, off)
    set_option(eng, "conv_up_phase", 2)
    on = [check_case(eng, dev, s, 20 + i)[1] for i, s in enumerate(SHAPES)]
    return off, on


def check_stats(eng, dev, shape=SHAPES[0], seed=5):
    """(conv_up_phase = 2 set by the caller.)  The partial rows the epilogue writes, reduced per (image, channel), are the sum and the sum of squares of the stored output.  Bound: an fp32
    sum of n terms carried out in any order is within n * 2^-24 * sum|v| of the exact one (the squares carry one more rounding each); both sides
    are compared in float64, the right-hand side computed from the stored fp32 output."""
    N, H, W, Cin, Cout = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, H, W, Cin, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(Cin * 9)
    b = 0.1 * torch.randn(Cout, generator=g)
    eng.lib.kernel_counts(reset=True)
    out, stats = eng.op_conv_up_stats(x.to(dev), w.to(dev), b.to(dev))
    assert eng.lib.kernel_counts().get("conv_up_phase", 0) == 1, eng.lib.kernel_counts()
    out = out.cpu().double()
    ref = F.conv2d(F.interpolate(S.nchw(x), scale_factor=2.0, mode="nearest"), w, b, padding=1)
    assert (S.nchw(out.float()) - ref).abs().max().item() < 3e-4
    got = stats.cpu().double().sum(1)                                   # [N, Cout, 2]
    n = 4 * H * W
    s1, s2, sa = out.sum((1, 2)), (out * out).sum((1, 2)), out.abs().sum((1, 2))
    e1 = ((got[..., 0] - s1).abs() / (n * 2.0 ** -24 * sa)).max().item()
    e2 = ((got[..., 1] - s2).abs() / ((n + 2) * 2.0 ** -24 * s2)).max().item()
    print(f"[up-phase statistics] error / bound: sum {e1:.3f}, sum of squares {e2:.3f}")
    assert e1 <= 1.0 and e2 <= 1.0, (e1, e2)
