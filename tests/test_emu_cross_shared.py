"""Cross-attention on ONE key / value operand per forward (option cross_shared) on the kernel emulator: the patch planes of the
trimap latent, the two host-folded Linears (q_shared / out_shared), one whole cross-attention against the unfolded fp64 computation of the
reference graph (aux_conv_in -> to_k / to_v, meta_arch.py:215-218), and the forward end to end with its launch census."""
import ctypes
import math
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from test_emu_folds import _engine, _setup      # noqa: E402  (the tiny architecture with non-zero folded biases)

TOL = 1e-3
SCALE = (64 ** -0.5) * math.log2(math.e)        # softmax(q.k * d^-1/2) evaluated as 2^(q'.k - max): folded into to_q / q_shared
BLOCKS = ["unet.down_blocks.0.attentions.0", "unet.mid_block.attentions.0", "unet.up_blocks.3.attentions.2"]
N_TRANSFORMER_BLOCKS = 16                       # 3 levels x 2 down, 1 mid, 3 levels x 3 up


def _weights():
    cfg, w = _setup()
    g = torch.Generator().manual_seed(6)
    for k in list(w):
        if k.endswith("attn2.to_out.0.bias"):
            w[k] = torch.randn(w[k].shape, generator=g) * 0.1
    return cfg, w


def _uin(z):
    """The 16-channel NHWC U-Net input tensor with the trimap latent z [B,4,H,W] at channels 4..7 (other channels: noise the kernel must not read)."""
    B, _, H, W = z.shape
    x16 = torch.randn(B, H, W, 16, generator=torch.Generator().manual_seed(3))
    x16[..., 4:8] = z.permute(0, 2, 3, 1)
    return x16


def _pair_plane(x):
    """Python restatement of the pair plane (k_attn.h, PREC = 3): per 4 channels [e5m2(y) x 4 | e5m2((y - fp16(y)) * 2^11) x 4], y clamped to the largest
    finite e5m2; x fp32 [..., 64] -> uint8 [..., 64, 2] (the bytes at the addresses of the fp16 elements)."""
    y = x.clamp(-57344.0, 57344.0)
    lo = (y - y.half().float()) * 2048.0
    a = y.to(torch.float8_e5m2).view(torch.uint8).reshape(*x.shape[:-1], 16, 4)
    b = lo.to(torch.float8_e5m2).view(torch.uint8).reshape(*x.shape[:-1], 16, 4)
    return torch.cat([a, b], dim=-1).reshape(*x.shape[:-1], 64, 2)


def _folded_tables(w, p):
    """fp64: wf_k / wf_v [C][36] (j = ci*9 + tap) and bk / bv [C] of block prefix p (fold_cross_kv)."""
    wa = w["unet.aux_conv_in.weight"].double().reshape(-1, 36)             # [ctx][36]
    ba = w["unet.aux_conv_in.bias"].double()
    wk, wv = w[p + ".to_k.weight"].double(), w[p + ".to_v.weight"].double()
    return wk @ wa, wv @ wa, wk @ ba, wv @ ba


def test_patch_planes_are_the_unfolded_latent(pkg):
    cfg, w = _weights()
    eng = _engine(cfg, w, "fp16x3")
    g = torch.Generator().manual_seed(21)
    for shape in ((2, 4, 8, 8), (1, 4, 8, 16)):
        z = torch.randn(shape, generator=g)
        B, _, H, W = shape
        L = H * W
        k_hi, k_pair, vt = eng.op_cross_patch_planes(_uin(z))
        P = F.unfold(z, 3, padding=1).permute(0, 2, 1).contiguous()        # [B, L, 36], column = ci*9 + ky*3 + kx
        assert torch.equal(k_hi[:, :, :36], P.half()), shape
        assert bool((k_hi[:, :, 36:] == 0).all()), shape
        assert vt.shape == (B, 64, (L + 63) // 64 * 64) and torch.equal(vt[:, :, :L], k_hi.transpose(1, 2)), shape
        assert bool((vt[:, :, L:] == 0).all()), shape
        P64 = torch.zeros(B, L, 64)
        P64[:, :, :36] = P
        assert torch.equal(k_pair, _pair_plane(P64)), shape
    eng.close()


def test_q_shared_and_out_shared_equal_the_folded_expressions(pkg):
    cfg, w = _weights()
    eng = _engine(cfg, w, "fp16x3")
    g = torch.Generator().manual_seed(22)
    for b in BLOCKS:
        p = b + ".transformer_blocks.0.attn2"
        C = w[p + ".to_q.weight"].shape[0]
        heads = C // 64
        wfk, wfv, _, bv = _folded_tables(w, p)
        wq, wo, bo = w[p + ".to_q.weight"].double(), w[p + ".to_out.0.weight"].double(), w[p + ".to_out.0.bias"].double()
        Wq = torch.zeros(C, C, dtype=torch.float64)
        Wo = torch.zeros(C, C, dtype=torch.float64)
        for h in range(heads):
            s = slice(h * 64, h * 64 + 64)
            Wq[h * 64:h * 64 + 36] = SCALE * wfk[s].T @ wq[s]              # [36][C]: sum_d wf_k[h*64+d][j] Wq[h*64+d][c]
            Wo[:, h * 64:h * 64 + 36] = wo[:, s] @ wfv[s]                  # [C][36]: sum_d Wo[c][h*64+d] wf_v[h*64+d][j]
        bias = bo + wo @ bv
        x = torch.randn(1, 4, 4, C, generator=g)
        want_q = F.linear(x.double(), Wq)
        got_q = eng.debug_run_layer(p + ".q_shared", x, C)
        eq = (got_q - want_q).abs().max().item() / want_q.abs().max().item()
        r = torch.randn(1, 4, 4, C, generator=g)
        want_o = F.linear(r.double(), Wo, bias)
        got_o = eng.debug_run_layer(p + ".out_shared", r, C)
        eo = (got_o - want_o).abs().max().item() / want_o.abs().max().item()
        print(f"[cross_shared] {b}: q_shared rel err {eq:.2e}, out_shared rel err {eo:.2e}")
        assert eq < 2e-5 and eo < 2e-5, (b, eq, eo)
        for h in range(heads):                                             # the 28 padding columns / rows of every head are exactly zero
            assert bool((got_q[..., h * 64 + 36:h * 64 + 64] == 0).all()), b
    eng.close()


def test_whole_cross_attention_equals_the_unfolded_reference(pkg, engine_option):
    cfg, w = _weights()
    eng = _engine(cfg, w, "fp16x3")
    g = torch.Generator().manual_seed(23)
    b = "unet.mid_block.attentions.0"
    p = b + ".transformer_blocks.0.attn2"
    C = w[p + ".to_q.weight"].shape[0]
    heads = C // 64
    z = torch.randn(2, 4, 8, 8, generator=g)
    x = torch.randn(2, 8, 8, C, generator=g)
    ctx = F.conv2d(z.double(), w["unet.aux_conv_in.weight"].double(), w["unet.aux_conv_in.bias"].double(), padding=1)
    tokens = ctx.permute(0, 2, 3, 1).reshape(2, 64, -1)
    q = F.linear(x.double().reshape(2, 64, C), w[p + ".to_q.weight"].double()).view(2, 64, heads, 64).transpose(1, 2)
    k = F.linear(tokens, w[p + ".to_k.weight"].double()).view(2, 64, heads, 64).transpose(1, 2)
    v = F.linear(tokens, w[p + ".to_v.weight"].double()).view(2, 64, heads, 64).transpose(1, 2)
    o = torch.softmax(q @ k.transpose(-1, -2) / 8.0, dim=-1) @ v
    want = F.linear(o.transpose(1, 2).reshape(2, 64, C), w[p + ".to_out.0.weight"].double(), w[p + ".to_out.0.bias"].double()).view(2, 8, 8, C)
    errs = {}
    for opt in (1, 0):
        engine_option(eng, "cross_shared", opt)
        eng.lib.kernel_counts(reset=True)
        got = eng.debug_cross_attention(b, x, _uin(z))
        counts = eng.lib.kernel_counts()
        assert counts.get("cross_patch_planes", 0) == opt and counts.get("transpose_v", 0) == 1 - opt, (opt, counts)
        errs[opt] = (got - want).abs().max().item() / want.abs().max().item()
    print(f"[cross_shared] whole cross-attention rel err: shared {errs[1]:.2e}, per-block K|V {errs[0]:.2e}")
    assert errs[1] < 1e-3 and errs[0] < 1e-3, errs
    eng.close()


def test_forward_end_to_end_and_launch_census(pkg, engine_option):
    from comfyui_sdmatte_amd.synth import synthetic_inputs
    from oracle import sdmatte_oracle as O
    cfg, w = _weights()
    img, tri = synthetic_inputs(2, 64, 64, seed=4)
    ref, _ = O.apply_matte(w, cfg.as_dict(), img, tri, 64, mask_refine=False)
    eng = _engine(cfg, w, "fp16x3")
    alpha, counts = {}, {}
    for opt in (1, 0):
        engine_option(eng, "cross_shared", opt)
        eng.lib.kernel_counts(reset=True)
        alpha[opt] = eng.apply_matte(img, tri, 64)
        counts[opt] = eng.lib.kernel_counts()
        d = (alpha[opt] - ref).abs().max().item()
        print(f"[cross_shared] end to end, cross_shared = {opt}: max |alpha - oracle| = {d:.3e}")
        assert d <= TOL, (opt, d)
    print(f"[cross_shared] max |alpha(1) - alpha(0)| = {(alpha[1] - alpha[0]).abs().max().item():.3e}")
    assert counts[1].get("cross_patch_planes", 0) == 1 and counts[0].get("cross_patch_planes", 0) == 0, (counts[1], counts[0])
    assert counts[0]["transpose_v"] - counts[1]["transpose_v"] == N_TRANSFORMER_BLOCKS, (counts[1], counts[0])
    assert counts[0]["conv3x3_thin"] - counts[1]["conv3x3_thin"] == N_TRANSFORMER_BLOCKS, (counts[1], counts[0])
    eng.close()
