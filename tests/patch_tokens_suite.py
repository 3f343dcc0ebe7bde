"""Shared checks of the patch token order of the U-Net transformers (engine option attn_patch_tokens) for the emulator and the GPU:
the helper pair against a numpy restatement, the way in (GroupNorm -> operand planes of proj_in), the way out (the proj_out epilogue of the plane-fed GEMM:
rows, residual, statistics, borders), and the level's key bias with the list of active key tiles built from it."""
import numpy as np
import torch

GUARD = 64          # guard rows in front of and behind the output of the way-out launches


def rule_np(H, W):
    return H % 8 == 0 and W % 8 == 0 and W >= 64


def token_of_pixel_np(H, W):
    """token of pixel (y, x), as the issue states it, for one H x W image -> int64 [H*W] (index = y * W + x)."""
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    return ((((y >> 3) * (W >> 3) + (x >> 3)) * 64) + (y & 7) * 8 + (x & 7)).reshape(-1)


def pixel_of_token_np(H, W):
    t = token_of_pixel_np(H, W)
    p = np.empty_like(t)
    p[t] = np.arange(H * W)
    return p


def check_map(eng):
    for (H, W) in ((8, 64), (16, 64), (24, 72)):
        on, t_of_p, p_of_t = eng.patch_token_map(H, W)
        assert on and rule_np(H, W), (H, W)
        want = token_of_pixel_np(H, W)
        assert np.array_equal(t_of_p, want), (H, W)
        assert np.array_equal(np.sort(t_of_p), np.arange(H * W)), (H, W)                 # a bijection ...
        assert np.array_equal(p_of_t[t_of_p], np.arange(H * W)), (H, W)                  # ... and the second helper is its inverse
        assert np.array_equal(p_of_t, pixel_of_token_np(H, W)), (H, W)
        # 64 consecutive tokens are one 8 x 8 patch
        py, px = p_of_t // W, p_of_t % W
        for t0 in range(0, H * W, 64):
            assert py[t0:t0 + 64].max() - py[t0:t0 + 64].min() == 7 and px[t0:t0 + 64].max() - px[t0:t0 + 64].min() == 7, (H, W, t0)
    for (H, W) in ((16, 32), (12, 64), (16, 68)):
        on, t_of_p, p_of_t = eng.patch_token_map(H, W)
        assert not on and not rule_np(H, W), (H, W)
        assert np.array_equal(t_of_p, np.arange(H * W)) and np.array_equal(p_of_t, np.arange(H * W)), (H, W)


def _perm_rows(N, H, W, dev):
    """index tensor P with token-order rows = pixel-order rows[P] (B = N images: the map is applied inside each image)."""
    p = torch.from_numpy(pixel_of_token_np(H, W))
    return torch.cat([p + n * H * W for n in range(N)]).to(dev)


def _planes_rows(raw, rows, C):
    """Raw P3 planes -> (hi [rows_pad, C] int16 view, xl [rows_pad, C] uint8) in logical (row, channel) order."""
    rows_pad = (rows + 31) // 32 * 32
    hi = raw[:rows_pad * C * 2].view(torch.int16).view(rows_pad // 16, C // 32, 4, 16, 8)          # [row block][channel chunk][granule][row][8 halves]
    hi = hi.permute(0, 3, 1, 2, 4).reshape(rows_pad, C)
    xl = raw[rows_pad * C * 2:].view(rows_pad // 32, C // 32, 2, 32, 16)                            # [row block][chunk][half][row][16 bytes]
    xl = xl.permute(0, 3, 1, 2, 4).reshape(rows_pad, C)
    return hi, xl


def check_way_in(eng, dev):
    g = torch.Generator().manual_seed(11)
    N = 2
    for (H, W) in ((8, 64), (24, 72)):
        for C in (32, 320):
            x = (torch.randn(N, H, W, C, generator=g) * 1.5 + 0.3).to(dev)
            gamma, beta = (torch.randn(C, generator=g) * 0.5 + 1.0).to(dev), (torch.randn(C, generator=g) * 0.2).to(dev)
            a, b = eng.op_groupnorm_p3(x, gamma, beta, 1e-6, groups=32)      # (one statistics pass for both: its atomics make two passes differ in the last bit)
            rows = N * H * W
            ahi, axl = _planes_rows(a, rows, C)
            bhi, bxl = _planes_rows(b, rows, C)
            P = _perm_rows(N, H, W, dev)
            assert torch.equal(bhi[:rows], ahi[:rows][P]) and torch.equal(bxl[:rows], axl[:rows][P]), (H, W, C)
            assert not torch.equal(bhi[:rows], ahi[:rows]), (H, W, C)                         # (the permutation is not the identity)
            # rows of the padding up to a multiple of 32: as before (N * H * W is a multiple of 32 at both sizes: there are none; the plane sizes agree)
            assert a.numel() == b.numel() and torch.equal(ahi[rows:], bhi[rows:]) and torch.equal(axl[rows:], bxl[rows:]), (H, W, C)


def _way_out_case(eng, dev, H, W, O, mode, seed):
    g = torch.Generator().manual_seed(seed)
    N, K = 2, 64
    rows = N * H * W
    x = torch.randn(N, H, W, K, generator=g).to(dev)
    w = (torch.randn(O, K, generator=g) / 8.0).to(dev)
    bias = (torch.randn(O, generator=g) * 0.1).to(dev)
    res = torch.randn(N, H, W, O, generator=g).to(dev)                                       # pixel order, different at every pixel
    P = _perm_rows(N, H, W, dev)                                                             # token r of the batch -> pixel row P[r]
    # the unmapped launch: row r gets the residual of row r, so give it the residual of token r's pixel
    res_tok = res.reshape(rows, O)[P].reshape(N, H, W, O).contiguous()
    eng.lib.kernel_counts(reset=True)
    plain = eng.op_gemm_p3_tokens(x, w, bias, mode=mode, res=res_tok, patch_tokens=False)
    c0 = eng.lib.kernel_counts()
    assert c0.get("gemm_p3", 0) == 1 and c0.get("gemm_p3_tokens", 0) == 0, c0
    buf = torch.full((rows + 2 * GUARD, O), 12345.0, dtype=torch.float32, device=dev)
    out_view = buf[GUARD:GUARD + rows].view(N, H, W, O)
    eng.lib.kernel_counts(reset=True)
    mapped = eng.op_gemm_p3_tokens(x, w, bias, mode=mode, res=res, patch_tokens=True, out=out_view)
    c1 = eng.lib.kernel_counts()
    assert c1.get("gemm_p3_tokens", 0) == 1, c1                                              # the instantiation that ran
    if mode == 4:
        plain, st_plain = plain
        mapped, st = mapped
    # rows of the unmapped launch put in pixel order
    want = torch.empty(rows, O, dtype=torch.float32, device=dev)
    want[P] = plain.reshape(rows, O)
    assert torch.equal(mapped.reshape(rows, O), want), (H, W, O, mode)
    # the guard rows in front of and behind the output keep their pattern
    assert bool((buf[:GUARD] == 12345.0).all()) and bool((buf[GUARD + rows:] == 12345.0).all()), (H, W, O, mode)
    if mode == 4:
        # per image and channel: sum of the partial rows against an fp64 sum of the output
        got = st.double().sum(dim=1)                                                          # [N, O, 2]
        o64 = mapped.reshape(N, H * W, O).double()
        s1, s2 = o64.sum(dim=1), (o64 * o64).sum(dim=1)
        # relative to the sum of magnitudes, the quantity an fp32 summation's error is proportional to (the signed sum of a channel may cancel to anything)
        e1 = ((got[..., 0] - s1).abs() / o64.abs().sum(dim=1)).max().item()
        e2 = ((got[..., 1] - s2).abs() / s2).max().item()
        print(f"[patch tokens, way out {H}x{W} O={O}] statistics rel err: sum {e1:.2e}, sumsq {e2:.2e}")
        assert e1 < 1e-6 and e2 < 1e-6, (H, W, O, e1, e2)
        assert st.shape == st_plain.shape


def check_way_out(eng, dev, mode, shape, O):
    _way_out_case(eng, dev, shape[0], shape[1], O, mode, 100 + mode * 10 + O)


def disc_plane(B, S, radius_frac=0.3):
    """trimap plane [-1, 1] of a centred disc of radius radius_frac * S on S x S."""
    y, x = np.meshgrid(np.arange(S), np.arange(S), indexing="ij")
    c = (S - 1) / 2.0
    m = (((y - c) ** 2 + (x - c) ** 2) <= (radius_frac * S) ** 2).astype(np.float32)
    return torch.from_numpy(np.repeat((m * 2 - 1)[None], B, axis=0).copy())


def tiles_np(bias_row, margin=2000.0):
    """numpy restatement of the engine's list: 64-key tiles holding a key within `margin` of the largest bias."""
    Lk = bias_row.shape[0]
    lim = bias_row.max() - margin
    return [t for t in range((Lk + 63) // 64) if bias_row[t * 64:(t + 1) * 64].max() >= lim]


def check_bias_and_list(eng, dev):
    S, B = 512, 2                                                        # level 0: a 64 x 64 latent
    plane = disc_plane(B, S)
    plane[1] = torch.roll(plane[1], (37, -51), (0, 1))                   # the second image: the disc off centre
    plane = plane.to(dev)
    hook = eng.op_mask_bias(plane, 0).cpu()                              # row-major, natural-log domain
    tok, on = eng.op_mask_bias_tokens(plane, 0, True)
    row, on0 = eng.op_mask_bias_tokens(plane, 0, False)
    assert on and not on0
    log2e = np.float32(1.4426950408889634)
    assert torch.equal(row.cpu(), (hook * log2e))                        # the same values, log2 domain
    P = torch.from_numpy(pixel_of_token_np(64, 64))
    assert torch.equal(tok.cpu(), row.cpu()[:, P])                       # token order = the row-major bias permuted, exactly
    lt, lr = eng.op_active_tiles(tok).cpu().numpy(), eng.op_active_tiles(row).cpu().numpy()
    for b in range(B):
        wt, wr = tiles_np(tok[b].cpu().numpy()), tiles_np(row[b].cpu().numpy())
        assert lt[b, 0] == len(wt) and list(lt[b, 1:1 + len(wt)]) == wt, b
        assert lr[b, 0] == len(wr) and list(lr[b, 1:1 + len(wr)]) == wr, b
        print(f"[patch tokens] 64x64 disc, image {b}: {len(wt)} active 8x8 tiles, {len(wr)} active strips of 64")
    # centred disc of radius 0.3 W: the 8 x 8 list is shorter than the strip list, by numpy's counts
    n_patch, n_strip = len(tiles_np(tok[0].cpu().numpy())), len(tiles_np(row[0].cpu().numpy()))
    assert n_patch < n_strip and lt[0, 0] == n_patch and lr[0, 0] == n_strip, (n_patch, n_strip)
    # a level that fails the rule keeps row-major order whatever the flag (level 1: 32 x 32)
    t1, on1 = eng.op_mask_bias_tokens(plane, 1, True)
    r1, _ = eng.op_mask_bias_tokens(plane, 1, False)
    assert not on1 and torch.equal(t1, r1)
