"""The GroupNorm statistics chain at operator level, shared by the emulator tests and the GPU tests: conv / GEMM epilogues write partial {sum, sumsq}
rows (one per (tile, wave row) of an image; split-K: one per 64 rows), gn_partials_scale_shift_kernel (csrc/k_norm.h) reduces them to the per-channel
scale | shift table, the next conv applies the table inside its operand staging.  Three checks:
  check_partials  a producer's rows against the sum and the sum of squares of the output it STORED, with the row buffer poisoned (option
                  dbg_stats_poison: the buffers are never cleared, a row that a launch geometry forgets would be stale arena memory);
  check_reducer   the reducer alone on synthetic rows against a float64 reduction of the same rows;
  check_chain     producer -> reducer -> consumer with the real kernels on both sides (sdm_op_conv_stats with the producer's rows as input statistics).
Tolerances: the statistics bound is up_phase_suite.check_stats's (an fp32 sum of n terms in any order is within n * 2^-24 * sum|v| of the exact one, the
squares carry one more rounding each); conv outputs meet ops_suite.check_conv's bar for their arithmetic (4e-3 fp16 operands, 3e-5 fp16x3, 3e-4 F8)."""
import math

import torch
import torch.nn.functional as F

import ops_suite as S

# (TH, TW, wave rows) of the tile configurations (sdm_engine.cpp kCfg3s1 / kCfg3s2; 1x1: rows per tile, wave rows)
CFG_3S1 = [(8, 32, 2), (4, 32, 4), (8, 8, 2), (16, 32, 4), (8, 32, 4), (8, 32, 2)]
CFG_3S2 = [(4, 32, 4), (8, 8, 2), (4, 32, 2), (8, 32, 4)]
CFG_1 = [(256, 2), (128, 4), (64, 2), (64, 2), (256, 2)]
CONV_COUNTERS = ("conv3x3_f8", "conv3x3_f8<gn>", "conv3x3_pc", "gemm_f8", "conv3x3_splitk", "gemm_splitk", "conv_up_phase", "conv3x3_f8_const_tiles", "gemm_p3")

RATIOS = {}      # family -> [max sum error / bound, max sum-of-squares error / bound] over the cases run so far (the tests print it)


def _cdiv(a, b):
    return -(-a // b)


def expected_srows(ntaps, stride, cfg, Ho, Wo, ksplit=1):
    if ksplit > 1:
        return _cdiv(Ho * Wo, 64)
    if ntaps == 9:
        th, tw, wm = (CFG_3S1 if stride == 1 else CFG_3S2)[cfg]
        return _cdiv(Ho, th) * _cdiv(Wo, tw) * wm
    bm, wm = CFG_1[cfg]
    return _cdiv(Ho * Wo, bm) * wm


def stats_vs_stored(out, stats, O, srows, family, tag):
    """out: the stored output [N, H, W, O] (any dtype), stats [N, srows', Cst, 2].  Every row the reducer will read was written by this launch (finite
    under the poison) and the rows summed per (image, channel) are the sums of the stored values, both sides in float64."""
    assert stats.shape[1] == srows, f"{tag}: {stats.shape[1]} partial rows per image, expected {srows}"
    st = stats.cpu()[..., :O, :]
    bad = (~torch.isfinite(st)).nonzero()
    assert bad.numel() == 0, f"{tag}: {bad.shape[0]} statistics values were not written by the launch, first (image, row, channel, which) = {bad[0].tolist()}"
    out = out.cpu().double()
    n = out.shape[1] * out.shape[2]
    got = st.double().sum(1)                                             # [N, O, 2]
    s1, s2, sa = out.sum((1, 2)), (out * out).sum((1, 2)), out.abs().sum((1, 2))
    e1 = ((got[..., 0] - s1).abs() / (n * 2.0 ** -24 * sa)).max().item()
    e2 = ((got[..., 1] - s2).abs() / ((n + 2) * 2.0 ** -24 * s2)).max().item()
    print(f"[gn chain / {family}] {tag}: error / bound: sum {e1:.3f}, sum of squares {e2:.3f}")
    r = RATIOS.setdefault(family, [0.0, 0.0])
    r[0], r[1] = max(r[0], e1), max(r[1], e2)
    assert e1 <= 1.0 and e2 <= 1.0, (tag, e1, e2)
    return e1, e2


# ---- producers -----------------------------------------------------------------------------------------------------------------------------------
F8 = dict(tile_cfg=0, in_f32=True, out_f32=True, split=True, f8=True, atol=3e-4)
X3 = dict(in_f32=True, out_f32=True, split=True, f8=False, atol=3e-5)          # fp16x3: split operands, residual terms on fp16
H16 = dict(atol=4e-3)                                                          # fp16 operands, fp16 output: the statistics are those of the rounded values


def producer_cases():
    """name -> (family, check_conv arguments, engine options, launch counter that must read 1 (None: a register-staged kernel - no conv counter moves),
    split-K factor)"""
    c = {}
    full = dict(N=2, H=16, W=64, Cin=64, Cout=128, res="f32", **F8)             # every tile full: the register-direct epilogue (DPP row adds on hardware)
    ragged = dict(N=2, H=12, W=40, Cin=64, Cout=160, **F8)                      # ragged bottom / right tiles, second channel tile 32 of 128 valid: both epilogues in one launch
    for epi in (4, 0, 3):
        c[f"f8_full_epi{epi}"] = ("F8 3x3", dict(full, seed=300 + epi), {"conv_epi": epi}, "conv3x3_f8", 1)
        c[f"f8_ragged_epi{epi}"] = ("F8 3x3", dict(ragged, seed=310 + epi), {"conv_epi": epi}, "conv3x3_f8", 1)
    # 12 tiles of 128 channels on a grid of 16 virtual tiles: with three tiles per block every block of the persistent grid runs two
    c["f8_tpb3"] = ("F8 3x3", dict(N=2, H=16, W=96, Cin=64, Cout=128, seed=320, **F8), {"conv_f8_tpb": 3}, "conv3x3_f8", 1)
    c["f8_concat"] = ("F8 3x3", dict(N=2, H=12, W=40, Cin=32, C1=32, Cout=128, res="f32", seed=321, **F8), {}, "conv3x3_f8", 1)
    # image-aligned tiles: 672 rows per image = two full 256-row tiles and a ragged one, in each of three images
    c["gemm_f8"] = ("F8 GEMM", dict(N=3, H=28, W=24, Cin=64, Cout=160, ntaps=1, res="f32", seed=330, **dict(F8, tile_cfg=4)), {}, "gemm_f8", 1)
    for cfg in (1, 2, 3, 5):
        prec = X3 if cfg != 3 else dict(out_f32=True, atol=4e-3)               # (the 512-pixel double-buffered tile has no split-precision form)
        c[f"s1_cfg{cfg}_f32"] = ("register-staged", dict(N=2, H=9, W=35, Cin=64, Cout=96, tile_cfg=cfg, res="f32", seed=340 + cfg, **prec), {}, None, 1)
        # fp16 output at 5 x 19: the bound grows with n^2, the difference between the sums of the rounded and of the un-rounded values with sqrt(n) - at
        # 95 pixels statistics taken in front of the rounding miss the bound, at 315 they would not
        c[f"s1_cfg{cfg}_f16"] = ("register-staged fp16 out", dict(N=2, H=5, W=19, Cin=64, Cout=96, tile_cfg=cfg, res="f16", seed=350 + cfg, **H16), {}, None, 1)
    for cfg in (0, 1, 2, 3):
        for pad in (0, 1):
            kw = dict(N=2, H=18, W=70, Cin=64, Cout=96, stride=2, pad_mode=pad, tile_cfg=cfg)      # (the engine's stride-2 convs take even sizes) -> 9 x 35
            c[f"s2_cfg{cfg}_pad{pad}_f32"] = ("register-staged", dict(kw, seed=360 + 2 * cfg + pad, **X3), {}, None, 1)
            c[f"s2_cfg{cfg}_pad{pad}_f16"] = ("register-staged fp16 out", dict(kw, H=10, W=38, seed=370 + 2 * cfg + pad, **H16), {}, None, 1)      # -> 5 x 19
    # split-K: 99 rows per image (one full 64-row block and a ragged one), 96 channels = a full and a ragged 64-channel block of the reduce kernel
    sk = dict(N=2, H=9, W=11, Cout=96)
    c["splitk_3x3_k2_f32_res"] = ("split-K", dict(sk, Cin=64, tile_cfg=2, res="f32", seed=380, **X3), {"conv_splitk": 2}, "conv3x3_splitk", 2)
    c["splitk_3x3_k4_f16"] = ("split-K fp16 out", dict(sk, Cin=64, tile_cfg=2, seed=381, **H16), {"conv_splitk": 4}, "conv3x3_splitk", 4)
    c["splitk_1x1_k4_f32"] = ("split-K", dict(sk, Cin=64, ntaps=1, tile_cfg=3, seed=382, **X3), {"conv_splitk": 4}, "gemm_splitk", 4)
    c["splitk_1x1_k2_f16_res"] = ("split-K fp16 out", dict(sk, Cin=128, ntaps=1, tile_cfg=2, res="f16", seed=383, **H16), {"conv_splitk": 2}, "gemm_splitk", 2)
    return c


PRODUCERS = producer_cases()


def check_partials(eng, dev, set_option, name):
    family, kw, opts, counter, ksplit = PRODUCERS[name]
    set_option(eng, "dbg_stats_poison", 1)
    for k, v in opts.items():
        set_option(eng, k, v)
    box = {}

    def op(x0, w, b, geglu=False, **a):
        box["out"], box["stats"] = eng.op_conv_stats(x0, w, b, **a)
        return box["out"]

    eng.lib.kernel_counts(reset=True)
    err = S.check_conv(eng, dev, op=op, **kw)                     # the output against check_conv's reference at check_conv's tolerance
    counts = {k: v for k, v in eng.lib.kernel_counts().items() if k in CONV_COUNTERS}
    assert counts == ({counter: 1} if counter else {}), (name, counts)
    ntaps, stride = kw.get("ntaps", 9), kw.get("stride", 1)
    Ho, Wo = (kw["H"], kw["W"]) if stride == 1 else (kw["H"] // 2, kw["W"] // 2)
    srows = expected_srows(ntaps, stride, kw["tile_cfg"], Ho, Wo, ksplit)
    e1, e2 = stats_vs_stored(box["out"], box["stats"], kw["Cout"], srows, family, name)
    return err, e1, e2


def check_const_tiles(eng, dev, set_option):
    """The representative tile's rows copied by const_tile_fill_kernel: the statistics of the launch with the class plane are bit-identical to those of the
    launch that multiplies every tile, and both are the sums of the stored output (inputs of ops_suite.check_conv_const_tiles, no GroupNorm in front)."""
    cls, x, w, b, _, r = S.const_tiles_inputs(gn=False)
    set_option(eng, "dbg_stats_poison", 1)
    set_option(eng, "conv_f8", 1)
    set_option(eng, "trimap_skip_min_rows", 8)
    kw = dict(tile_cfg=0, split=True, out_f32=True, res=r.to(dev))
    eng.lib.kernel_counts(reset=True)
    full, st_full = eng.op_conv_stats(x.to(dev), w.to(dev), b.to(dev), **kw)
    assert eng.lib.kernel_counts().get("conv3x3_f8_const_tiles", 0) == 0
    skip, st_skip = eng.op_conv_stats(x.to(dev), w.to(dev), b.to(dev), cmask=cls.to(dev), **kw)
    counts = eng.lib.kernel_counts()
    assert counts.get("conv3x3_f8_const_tiles", 0) == 1 and counts.get("conv3x3_f8", 0) == 2, counts
    N, H, W, _ = x.shape
    srows = expected_srows(9, 1, 0, H, W)
    ref = F.conv2d(S.nchw(x), w, b, padding=1) + S.nchw(r)
    assert (S.nchw(full.cpu()) - ref).abs().max().item() < 3e-4
    stats_vs_stored(full, st_full, w.shape[0], srows, "constant tiles", "every tile multiplied")
    stats_vs_stored(skip, st_skip, w.shape[0], srows, "constant tiles", "constant tiles filled")
    assert torch.equal(full, skip)
    same = (st_full == st_skip).all(dim=3).all(dim=2)                  # [N, srows]
    assert bool(same.all()), f"partial rows differ with the class plane, first (image, row) = {(~same).nonzero()[0].tolist()}"


# ---- the reducer alone ---------------------------------------------------------------------------------------------------------------------------
def reducer_cases():
    """name -> dict(C0, C1, rows0, k0, rows1, k1, mean, std, clamp): source s has rows_s partial rows of k_s pixels each (rows0 * k0 == rows1 * k1 = HW)"""
    return {
        "tail_loop_only": dict(C0=64, rows0=3, k0=8),                                  # cpg 2: 3 items per group, none reaches the 4x-unrolled body
        "unrolled_and_tail": dict(C0=64, rows0=4101, k0=2),                            # cpg 2: 4101 items > 4 * 1024: one unrolled round of every thread, 5 items in the tail loop
        "vec1_cpg3": dict(C0=96, rows0=7, k0=4),                                       # odd channels per group: 8-byte loads
        "vec1_cpg5": dict(C0=160, rows0=7, k0=4),
        "straddle_vec2": dict(C0=40, C1=152, rows0=6, k0=4, rows1=8, k1=3),            # cpg 6: group 6 = channels 36 .. 41 lies across the concat boundary
        "straddle_vec1": dict(C0=40, C1=56, rows0=6, k0=4, rows1=8, k1=3),             # cpg 3: group 13 = channels 39 .. 41
        "unequal_rows": dict(C0=64, C1=64, rows0=4, k0=6, rows1=12, k1=2),
        "far_off_mean": dict(C0=64, rows0=9, k0=8, mean=30.0, std=0.5),
        "clamp": dict(C0=64, rows0=5, k0=4, clamp=True),
    }


REDUCERS = reducer_cases()


def check_reducer(eng, dev, name, N=3, groups=32, eps=1e-6):
    """Bounds from the kernel's arithmetic - float64 up to rstd, one rounding of rstd (and of the mean) to fp32, one fp32 multiply (and one subtraction):
    |scale - ref| <= 4 * 2^-24 * |ref|, |shift - ref| <= 4 * 2^-24 * (|beta| + |mean * scale|)."""
    c = dict(C1=0, rows1=0, k1=0, mean=0.3, std=1.7, clamp=False)
    c.update(REDUCERS[name])
    g = S._g(sum(map(ord, name)))
    C = c["C0"] + c["C1"]
    HW = c["rows0"] * c["k0"]
    assert c["C1"] == 0 or c["rows1"] * c["k1"] == HW
    base = torch.randn(N, 1, 1, C, generator=g)                       # a different mean per (image, channel): every group has its own result
    srcs = []
    for C_s, rows, k, lo in ((c["C0"], c["rows0"], c["k0"], 0), (c["C1"], c["rows1"], c["k1"], c["C0"])):
        if not C_s:
            continue
        if c["clamp"]:
            # one constant v per image with the squares scaled DOWN: sumsq / count = v^2 (1 - 2^-10) < mean^2, a negative variance that the kernel clamps to 0
            v = (3.0 + base[..., :1]).expand(N, rows, 1, C_s)[:, :, 0]
            st = torch.stack([k * v, k * v * v * (1 - 2.0 ** -10)], dim=-1)
        else:
            x = c["mean"] + base[..., lo:lo + C_s] + c["std"] * torch.randn(N, rows, k, C_s, generator=g)
            st = torch.stack([x.sum(2), (x * x).sum(2)], dim=-1)      # fp32 partial rows [N, rows, C_s, 2]
        srcs.append(st.float().contiguous())
    gamma = 1 + 0.2 * torch.randn(C, generator=g)
    beta = 0.1 * torch.randn(C, generator=g)
    scale, shift = eng.op_gn_partials(srcs[0].to(dev), gamma.to(dev), beta.to(dev), eps, HW, groups=groups, st1=srcs[1].to(dev) if len(srcs) > 1 else None)
    scale, shift = scale.cpu().double(), shift.cpu().double()
    # float64 reduction of the same rows
    tot = torch.cat([s.double().sum(1) for s in srcs], dim=1)          # [N, C, 2]
    cpg = C // groups
    cnt = float(HW * cpg)
    gs = tot.view(N, groups, cpg, 2).sum(2)
    mean = gs[..., 0] / cnt
    var = gs[..., 1] / cnt - mean * mean
    if c["clamp"]:
        assert bool((var < 0).all()), "the case is built to give a negative variance"
    else:
        assert bool((var > 0).all())
    var = var.clamp_min(0.0)
    rstd = 1.0 / torch.sqrt(var + torch.tensor(eps, dtype=torch.float32).double())
    mean_c, rstd_c = mean.repeat_interleave(cpg, dim=1), rstd.repeat_interleave(cpg, dim=1)
    ref_scale = rstd_c * gamma.double()
    ref_shift = beta.double() - mean_c * ref_scale
    u = 4 * 2.0 ** -24
    e_scale = ((scale - ref_scale).abs() / (u * ref_scale.abs())).max().item()
    e_shift = ((shift - ref_shift).abs() / (u * (beta.double().abs() + (mean_c * ref_scale).abs()))).max().item()
    print(f"[gn chain / reducer] {name}: error / bound: scale {e_scale:.3f}, shift {e_shift:.3f}")
    assert bool(torch.isfinite(scale).all()) and bool(torch.isfinite(shift).all()), name
    assert e_scale <= 1.0 and e_shift <= 1.0, (name, e_scale, e_shift)
    return e_scale, e_shift


# ---- producer -> reducer -> consumer -------------------------------------------------------------------------------------------------------------
def _produce(eng, dev, g, N, H, W, Cin, Cout, conv_f8, **kw):
    x = torch.randn(N, H, W, Cin, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(Cin * 9)
    b = 0.1 * torch.randn(Cout, generator=g)
    eng.lib.set_option("conv_f8", conv_f8)
    return eng.op_conv_stats(x.to(dev), w.to(dev), b.to(dev), **kw)


CHAINS = {
    # name -> (concat, consumer tile cfg, consumer Cout, conv_f8 for the consumer, tolerance, consumer's launch counter or None)
    "single_cfg0_f8": (False, 0, 128, 1, 3e-4, "conv3x3_f8<gn>"),
    "single_cfg5_x3": (False, 5, 96, 0, 3e-5, None),
    "single_cfg4_x3": (False, 4, 32, 0, 3e-5, None),
    "concat_cfg0_f8": (True, 0, 128, 1, 3e-4, "conv3x3_f8<gn>"),
}


def check_chain(eng, dev, set_option, name, eps=1e-6):
    """Producer(s) with the epilogue statistics -> gn_partials_scale_shift_kernel -> a fused-GroupNorm conv, against F.group_norm -> SiLU -> conv of the
    producers' STORED outputs in fp32 (the consumer's tolerance in check_conv), and against the same consumer with the stand-alone statistics kernel
    (2e-5 * max|ref|: two statistics passes, ops_suite.check_conv_const_tiles)."""
    concat, cfg, Cout, conv_f8, atol, counter = CHAINS[name]
    g = S._g(sum(map(ord, name)))
    set_option(eng, "dbg_stats_poison", 1)
    N, H, W = 2, 12, 44
    # source 0: the F8 3x3 kernel (full and ragged tiles), 4 tiles x 2 wave rows = 8 partial rows per image
    eng.lib.kernel_counts(reset=True)
    y0, st0 = _produce(eng, dev, g, N, H, W, 64, 128, 1, tile_cfg=0, split=True, out_f32=True)
    assert eng.lib.kernel_counts().get("conv3x3_f8", 0) == 1 and st0.shape[1] == 8, (eng.lib.kernel_counts(), st0.shape)
    y1 = st1 = None
    if concat:
        # the first 64 channels of source 0 and their partial rows, and a split-K conv with 9 rows per image as source 1
        y0, st0 = y0[..., :64].contiguous(), st0[..., :64, :].contiguous()
        set_option(eng, "conv_splitk", 2)
        y1, st1 = _produce(eng, dev, g, N, H, W, 64, 32, 0, tile_cfg=2, split=True, out_f32=True)
        set_option(eng, "conv_splitk", -1)
        assert eng.lib.kernel_counts().get("conv3x3_splitk", 0) == 1 and st1.shape[1] == 9, (eng.lib.kernel_counts(), st1.shape)
    C0, C1 = y0.shape[-1], (y1.shape[-1] if concat else 0)
    C = C0 + C1
    w = torch.randn(Cout, C, 3, 3, generator=g) / math.sqrt(C * 9)
    b = 0.1 * torch.randn(Cout, generator=g)
    gamma = 1 + 0.2 * torch.randn(C, generator=g)
    beta = 0.1 * torch.randn(C, generator=g)
    gn = (gamma.to(dev), beta.to(dev), eps, 32, True)
    kw = dict(x1=y1, tile_cfg=cfg, split=True, out_f32=True, gn=gn)
    eng.lib.set_option("conv_f8", conv_f8)
    eng.lib.kernel_counts(reset=True)
    got, _ = eng.op_conv_stats(y0, w.to(dev), b.to(dev), in_stats=(st0, st1) if concat else (st0,), **kw)
    counts = {k: v for k, v in eng.lib.kernel_counts().items() if k in CONV_COUNTERS}
    assert counts == ({counter: 1} if counter else {}), (name, counts)
    alone = eng.op_conv(y0, w.to(dev), b.to(dev), **kw)                  # statistics by gn_stats_kernel (atomics) + gn_finalize_kernel
    eng.lib.set_option("conv_f8", 1)
    ys = torch.cat([y0.cpu(), y1.cpu()], dim=-1) if concat else y0.cpu()
    ref = F.conv2d(F.silu(F.group_norm(S.nchw(ys), 32, gamma, beta, eps)), w, b, padding=1)
    got, alone = S.nchw(got.cpu()), S.nchw(alone.cpu())
    err = (got - ref).abs().max().item()
    d = (got - alone).abs().max().item() / ref.abs().max().item()
    print(f"[gn chain / chain] {name}: max|d| vs fp32 reference {err:.3e} (bar {atol:.0e}), vs stand-alone statistics {d:.3e} of max|ref| (bar 2e-5)")
    assert bool(torch.isfinite(got).all()), name
    assert err < atol, (name, err)
    assert d <= 2e-5, (name, d)
    return err, d
