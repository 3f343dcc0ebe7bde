// sdm_hooks.h - the part of the C ABI (include/sdmatte.h) that no product path calls: single-operator test hooks (sdm_op_*, sdm_debug_*) and
// lab / bench helpers (sdm_bench_*).  Included once, at the end of sdm_engine.cpp: one translation unit, every kernel compiled once.
#pragma once

struct DevBuf {      // a device allocation that is freed with its scope
  void* p = nullptr;
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p(o.p) { o.p = nullptr; }      // (move-only: this deletes the copies)
  ~DevBuf() { if (p) dev_free(p); }
  int alloc(size_t n) { return dev_malloc(&p, n); }
  int alloc0(size_t n, void* stream) { const int rc = alloc(n); return rc ? rc : dev_memset(p, 0, n, stream); }
};

struct RestoreInt { int& s; int v; ~RestoreInt() { s = v; } };      // RestoreInt keep{x, x}: x gets its present value back on every way out

// A layer outside the model: shape and layouts by the rules of the model's layers (make_layer / layer_choose_layouts), buffers of its own (zeroed,
// as the weight arena is), fp32 weights and bias (device) packed and derived by the model's path.  Released after the engine stream has drained.
struct TempLayer {
  enum { kDma = 1, kW3 = 2, kUp = 4 };      // layouts wanted: the stage-ordered 3x3 / fp8-residual GEMM copy of an eligible layer; W3; the phase matrices of an up-sampling 3x3 layer
  sdm_ctx* e;
  ConvL L;
  DevBuf w, w_lo, b, w_dma, w3, wup;
  explicit TempLayer(sdm_ctx* c) : e(c) {}
  ~TempLayer() { dev_sync(e->stream); }      // (then the buffers go)
  int init(const char* name, int ntaps, int I, int O, int geglu, int split, int layouts, const float* wsrc, const float* bias) {
    L = make_layer(name, ntaps, I, O, geglu, split);
    layer_choose_layouts(L, layouts & kDma, layouts & kDma, layouts & kW3, layouts & kUp);
    SDM_CHECK_DEV(e, w.alloc0(L.w_bytes(), e->stream));
    SDM_CHECK_DEV(e, b.alloc0(L.b_bytes(), e->stream));
    if (L.split) SDM_CHECK_DEV(e, w_lo.alloc0(L.w_bytes(), e->stream));
    if (L.wdma_bytes) SDM_CHECK_DEV(e, w_dma.alloc0(L.wdma_bytes, e->stream));
    if (L.w3_bytes) SDM_CHECK_DEV(e, w3.alloc0(L.w3_bytes, e->stream));
    if (L.wup_bytes) SDM_CHECK_DEV(e, wup.alloc0(L.wup_bytes, e->stream));
    L.wup = (unsigned char*)wup.p;
    L.w = (half_t*)w.p; L.b = (float*)b.p; L.w_lo = (half_t*)w_lo.p; L.w_dma = (half_t*)w_dma.p; L.w3 = (unsigned char*)w3.p;
    pack_layer_weight(e, L, wsrc, O, I, 0, 0, 1.0f);
    {   // The caller's weights are on the device, so this is a second form of sdm_load_tensor's range check (check_weight_range works on the host copy of a
        // checkpoint tensor and reports max|w|): a max over the packed high parts, where a weight beyond fp16 reads inf - it can say that one does not fit,
        // not which value.  One small launch, a 4-byte copy and a stream sync per hook call (the bench helpers that build a TempLayer pay it in front of
        // their timed launches, not inside them); derive_layers takes its own max only for the layers with an fp8 copy, after this point.
      DevBuf mx;
      SDM_CHECK_DEV(e, mx.alloc0(4, e->stream));
      const size_t n = L.w_bytes() / 2;
      unsigned int* mp = (unsigned int*)mx.p;
      SDM_LAUNCH(absmax_f16_kernel, dim3((unsigned)std::min<size_t>((n + 255) / 256, 2048)), dim3(256), 0, e->stream, (const half_t*)L.w, n, mp);
      float m = 0.0f;
      SDM_CHECK_DEV(e, dev_memcpy_d2h(&m, mp, 4, e->stream));
      SDM_CHECK_DEV(e, dev_sync(e->stream));
      if (!std::isfinite(m)) SDM_FAIL(e, SDM_ERR_INVALID, "%s: a weight does not fit the packed fp16 weight format (|w| * %g <= %g)", name, (double)ldexpf(1.0f, L.w_exp), (double)kK16Max);
    }
    if (bias) pack_layer_bias(e, L, bias, O, 0);
    std::vector<ConvL*> one{&L};
    return derive_layers(e, one);
  }
};

static T view(const void* p, int N, int H, int W, int C, int fmt) {      // a caller's buffer as an activation tensor (never tfree'd)
  T t;
  t.p = const_cast<void*>(p); t.N = N; t.H = H; t.W = W; t.C = C; t.f32 = fmt;
  return t;
}

#ifndef SDM_EMU
// ms per launch over `iters` launches between two events, behind one launch that is not timed
template <class F>
static float time_launches(sdm_ctx* e, int iters, F launch) {
  hipEvent_t e0, e1;
  (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
  launch();
  (void)hipEventRecord(e0, (hipStream_t)e->stream);
  for (int i = 0; i < iters; ++i) launch();
  (void)hipEventRecord(e1, (hipStream_t)e->stream);
  (void)hipEventSynchronize(e1);
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, e0, e1);
  (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
  return ms / (float)iters;
}
#endif

extern "C" {

// ---- single-operator entry points ----
int sdm_conv_num_cfgs(int ntaps, int stride) { return conv_num_cfgs(ntaps, stride); }

// One conv through op_conv, for sdm_op_conv_ex and sdm_op_conv_stats.  in_st0 (+ in_st1 for a concat): partial statistics rows of the input - the
// fused GroupNorm then takes its table from gn_partials_scale_shift_kernel as the model does, not from the stand-alone statistics kernel.
// stats: the output's own partial rows are wanted ([N][*srows][Cst][2], Cst = the stored channel count; room for stats_cap rows per image).
static int conv_hook(sdm_ctx* e, const void* in0, const void* in1, int C0, int C1, int in_f32, int N, int Hin, int Win, int up, int stride,
                     int pad_mode, int ntaps, const float* w, const float* bias, int O, void* out, int out_f32, const void* res, int res_f32,
                     int geglu, float out_scale, int tile_cfg, int split, const float* gn_gamma, const float* gn_beta, float gn_eps,
                     int gn_groups, int gn_silu, const float* in_st0, int in_rows0, const float* in_st1, int in_rows1, float* stats, int stats_cap,
                     int* srows) {
  if (e) dev_use(e->device);
  if (!e || !in0 || !w || !out) return SDM_ERR_INVALID;
  if (stats && !srows) return SDM_ERR_INVALID;
  if (in_st0 && (!gn_gamma || (in1 && !in_st1))) SDM_FAIL(e, SDM_ERR_INVALID, "sdm_op_conv_stats: input statistics go with a fused GroupNorm, one set of rows per source");
  if (C0 % 16 || C1 % 16) SDM_FAIL(e, SDM_ERR_INVALID, "sdm_op_conv: channel counts must be multiples of 16");
  if (split && !in_f32) SDM_FAIL(e, SDM_ERR_INVALID, "sdm_op_conv_ex: split precision takes fp32 activations");
  TempLayer tl(e);      // every layout a layer of this shape can carry but W3: the conv launchers never read it
  TRY(tl.init("op", ntaps, C0 + C1, O, geglu, split, TempLayer::kDma | (up ? TempLayer::kUp : 0), w, bias));
  const ConvL& L = tl.L;
  int Ho = Hin << up, Wo = Win << up;
  if (stride == 2) { Ho /= 2; Wo /= 2; }
  const int Cst = rup(geglu ? O / 2 : O, 4);   // rows are stored with 4-channel vectors
  T tin0 = view(in0, N, Hin, Win, C0, in_f32), tin1 = view(in1, N, Hin, Win, C1, in_f32);
  T tout = view(out, N, Ho, Wo, Cst, out_f32), tres = view(res, N, Ho, Wo, Cst, res_f32);
  if (e->dbg_cmask) { tin0.cmask = const_cast<unsigned char*>(e->dbg_cmask); tin0.cm_bytes = 1; e->dbg_cmask = nullptr; }      // (borrowed: tin0 is never tfree'd)
  ConvArgs a; a.in0 = &tin0; a.in1 = in1 ? &tin1 : nullptr; a.out = &tout; a.stride = stride; a.pad_mode = pad_mode; a.up = up;
  a.res = res ? &tres : nullptr; a.out_scale = out_scale; a.force_cfg = tile_cfg; a.cout_valid = Cst;
  tout.want_stats = stats != nullptr;
  if (gn_gamma) {
    // GroupNorm(+SiLU) of the input applied inside the conv's operand staging (the production path of every ResBlock conv): statistics by the
    // stand-alone kernel or from the caller's partial rows, scale/shift table, then the fused-GN instantiation of tile cfg 0 / 4 / 5
    if (ntaps != 9 || stride != 1 || up) SDM_FAIL(e, SDM_ERR_INVALID, "sdm_op_conv_ex: fused GroupNorm needs a 3x3 stride-1 conv");
    if (a.force_cfg != 0 && a.force_cfg != 4 && a.force_cfg != 5) a.force_cfg = (L.Cout_pad <= 32) ? 4 : 0;
  }
  RestoreInt keep_act{e->act_f32, e->act_f32};
  return run_two_pass(e, [&]() -> int {      // (the arena holds the split-K workspace, if the layer is split)
    T scratch;
    ConvArgs b = a;
    if (gn_gamma) {
      float* scale; float* shift;
      TRY(gn_scale_shift(e, in0, in1, C0, C1, in_f32, N, Hin * Win, gn_groups, gn_gamma, gn_beta, gn_eps, in_st0, in_rows0, in_st1, in_rows1,
                         in_st0 != nullptr, &scratch, &scale, &shift));
      b.gn_scale = e->dry ? (const float*)16 : scale; b.gn_shift = shift; b.gn_silu = gn_silu;
    }
    TRY(op_conv(e, L, b));
    if (stats && !e->dry) {
      if (tout.srows > stats_cap) SDM_FAIL(e, SDM_ERR_INVALID, "sdm_op_conv_stats: %d partial rows per image, room for %d", tout.srows, stats_cap);
      SDM_CHECK_DEV(e, dev_memcpy_d2d(stats, tout.stats, (size_t)N * tout.srows * Cst * 2 * 4, e->stream));
      *srows = tout.srows;
    }
    if (tout.sbytes) { tfree_raw(e, tout.soff, tout.sbytes); tout.sbytes = 0; }
    if (gn_gamma) tfree(e, scratch);
    return 0;
  });
}

int sdm_op_conv_ex(sdm_ctx* e, const void* in0, const void* in1, int C0, int C1, int in_f32, int N, int Hin, int Win, int up, int stride,
                   int pad_mode, int ntaps, const float* w, const float* bias, int O, void* out, int out_f32, const void* res, int res_f32,
                   int geglu, float out_scale, int tile_cfg, int split, const float* gn_gamma, const float* gn_beta, float gn_eps,
                   int gn_groups, int gn_silu) {
  return conv_hook(e, in0, in1, C0, C1, in_f32, N, Hin, Win, up, stride, pad_mode, ntaps, w, bias, O, out, out_f32, res, res_f32, geglu, out_scale,
                   tile_cfg, split, gn_gamma, gn_beta, gn_eps, gn_groups, gn_silu, nullptr, 0, nullptr, 0, nullptr, 0, nullptr);
}

/* sdm_op_conv_ex that also returns the partial {sum, sumsq} rows its epilogue writes for the next GroupNorm (`stats`, [N][*srows][Cst][2] with Cst = O
 * rounded up to 4; room for stats_cap rows per image) and, with in_st0 / in_rows0 (+ in_st1 / in_rows1 for a concat input) and gn_gamma, takes the fused
 * GroupNorm's scale | shift table from those rows through gn_partials_scale_shift_kernel - the chain every ResBlock conv of the model runs. */
int sdm_op_conv_stats(sdm_ctx* e, const void* in0, const void* in1, int C0, int C1, int in_f32, int N, int Hin, int Win, int up, int stride,
                      int pad_mode, int ntaps, const float* w, const float* bias, int O, void* out, int out_f32, const void* res, int res_f32,
                      int geglu, float out_scale, int tile_cfg, int split, const float* gn_gamma, const float* gn_beta, float gn_eps,
                      int gn_groups, int gn_silu, const float* in_st0, int in_rows0, const float* in_st1, int in_rows1, float* stats, int stats_cap,
                      int* srows) {
  if (!stats || !srows || stats_cap < 1) return SDM_ERR_INVALID;
  return conv_hook(e, in0, in1, C0, C1, in_f32, N, Hin, Win, up, stride, pad_mode, ntaps, w, bias, O, out, out_f32, res, res_f32, geglu, out_scale,
                   tile_cfg, split, gn_gamma, gn_beta, gn_eps, gn_groups, gn_silu, in_st0, in_rows0, in_st1, in_rows1, stats, stats_cap, srows);
}

/* The reducer alone: partial rows st0 [N][rows0][C0][2] (+ st1 [N][rows1][C1][2], the second source of a channel concat; C1 = 0: none) of images of HW pixels ->
 * scale [N][C0 + C1] = rstd * gamma and shift [N][C0 + C1] = beta - mean * rstd * gamma (gn_partials_scale_shift_kernel, as gn_scale_shift launches it). */
int sdm_op_gn_partials(sdm_ctx* e, const float* st0, int rows0, const float* st1, int rows1, int C0, int C1, int N, int HW, int groups,
                       const float* gamma, const float* beta, float eps, float* scale_out, float* shift_out) {
  if (e) dev_use(e->device);
  if (!e || !st0 || rows0 < 1 || (C1 > 0 && (!st1 || rows1 < 1)) || !gamma || !beta || !scale_out || !shift_out || N < 1 || HW < 1 || groups < 1) return SDM_ERR_INVALID;
  return run_two_pass(e, [&]() -> int {
    T scratch; float* scale; float* shift;
    TRY(gn_scale_shift(e, nullptr, nullptr, C0, C1, 1, N, HW, groups, gamma, beta, eps, st0, rows0, C1 > 0 ? st1 : nullptr, C1 > 0 ? rows1 : 0, true,
                       &scratch, &scale, &shift));
    if (!e->dry) {
      SDM_CHECK_DEV(e, dev_memcpy_d2d(scale_out, scale, (size_t)N * (C0 + C1) * 4, e->stream));
      SDM_CHECK_DEV(e, dev_memcpy_d2d(shift_out, shift, (size_t)N * (C0 + C1) * 4, e->stream));
    }
    tfree(e, scratch);
    return 0;
  });
}

/* The stand-alone statistics alone: x0 [N][HW][C0] (+ x1 [N][HW][C1], the second source of a channel concat; C1 = 0: none), fp32 or fp16 -> the scale | shift
 * tables of sdm_op_gn_partials, by gn_stats_kernel + gn_finalize_kernel as gn_scale_shift launches them for an input without partial rows. */
int sdm_op_gn_tables(sdm_ctx* e, const void* x0, const void* x1, int C0, int C1, int in_f32, int N, int HW, int groups, const float* gamma,
                     const float* beta, float eps, float* scale_out, float* shift_out) {
  if (e) dev_use(e->device);
  if (!e || !x0 || (C1 > 0 && !x1) || !gamma || !beta || !scale_out || !shift_out || N < 1 || HW < 1 || groups < 1) return SDM_ERR_INVALID;
  return run_two_pass(e, [&]() -> int {
    T scratch; float* scale; float* shift;
    TRY(gn_scale_shift(e, x0, C1 > 0 ? x1 : nullptr, C0, C1, in_f32, N, HW, groups, gamma, beta, eps, nullptr, 0, nullptr, 0, false, &scratch, &scale, &shift));
    if (!e->dry) {
      SDM_CHECK_DEV(e, dev_memcpy_d2d(scale_out, scale, (size_t)N * (C0 + C1) * 4, e->stream));
      SDM_CHECK_DEV(e, dev_memcpy_d2d(shift_out, shift, (size_t)N * (C0 + C1) * 4, e->stream));
    }
    tfree(e, scratch);
    return 0;
  });
}

/* Plane-fed GEMM (k_gemm.h) as a stand-alone operator: x fp32 [N*H*W][K] (device) is converted to P3 planes (to_p3_kernel, or LayerNorm with P3 output
 * when ln_gamma is given), w fp32 [O][K] is packed to K16 -> W3 exactly as a model layer.  mode 0: fp32 out (+bias, +fp32 residual); 1: GEGLU (O = 2 x outputs);
 * 3: linear (+residual) to P3; both P3 results are decoded to fp32 (hi + xl * 2^-11) into `out`; 2: raw q | k | v operand planes (fp16 hi [rows][O] then the
 * e5m2 pair plane, pair plane for channels < lo_cols only); 4: mode 0 + the consumer's GroupNorm statistics, [N][*srows][O][2] floats into `stats`. */
static int gemm_p3_hook(sdm_ctx* e, const float* x, int N, int H, int W, int K, const float* w, const float* bias, int O, int mode, const float* res,
                        const float* ln_gamma, const float* ln_beta, float ln_eps, int lo_cols, void* out, float* stats, int* srows, bool patch_tokens) {
  if (e) dev_use(e->device);
  if (!e || !x || !w || !out) return SDM_ERR_INVALID;
  const int geglu = mode == 1;
  if (K % 32 || O % (geglu ? 64 : 32)) SDM_FAIL(e, SDM_ERR_INVALID, "sdm_op_gemm_p3: K %% 32 and O %% 32 (GEGLU: 64) required");
  TempLayer tl(e);      // W3 alone: this hook is the plane-fed GEMM whatever K and O are
  TRY(tl.init("op_gemm_p3", 1, K, O, geglu, 1, TempLayer::kW3, w, bias));
  const ConvL& L = tl.L;
  const int Cst = geglu ? O / 2 : O;
  RestoreInt keep_act{e->act_f32, e->act_f32};
  e->act_f32 = 1;
  return run_two_pass(e, [&]() -> int {
    T tx = view(x, N, H, W, K, 1), tres = view(res, N, H, W, Cst, 1), xp, to;
    if (ln_gamma) {
      NormL nl; nl.C = K; nl.g = const_cast<float*>(ln_gamma); nl.b = const_cast<float*>(ln_beta);
      TRY(op_ln(e, nl, tx, ln_eps, &xp, kFmtP3));
    } else {
      TRY(op_to_p3(e, tx, &xp));
    }
    const bool planes = (mode == 1 || mode == 3);
    if (planes) to = talloc(e, N, H, W, Cst, kFmtP3);
    else to = view(out, N, H, W, Cst, (mode == 2) ? 3 : 1);
    to.want_stats = (mode == 4);
    TRY(op_gemm_p3(e, L, xp, &to, res ? &tres : nullptr, lo_cols, patch_tokens));
    if (!e->dry) {
      if (planes) SDM_LAUNCH(from_p3_kernel, dim3((unsigned)std::min<long>((to.rows() * Cst + 255) / 256, 1 << 20)), dim3(256), 0, e->stream, (const unsigned char*)to.p, (float*)out, to.rows(), Cst);
      if (mode == 4 && stats) {
        SDM_CHECK_DEV(e, dev_memcpy_d2d(stats, to.stats, (size_t)N * to.srows * Cst * 2 * 4, e->stream));
        if (srows) *srows = to.srows;
      }
    }
    if (planes) tfree(e, to);
    else if (to.sbytes) { tfree_raw(e, to.soff, to.sbytes); to.sbytes = 0; }
    tfree(e, xp);
    return 0;
  });
}

int sdm_op_gemm_p3(sdm_ctx* e, const float* x, int N, int H, int W, int K, const float* w, const float* bias, int O, int mode, const float* res,
                   const float* ln_gamma, const float* ln_beta, float ln_eps, int lo_cols, void* out, float* stats, int* srows) {
  return gemm_p3_hook(e, x, N, H, W, K, w, bias, O, mode, res, ln_gamma, ln_beta, ln_eps, lo_cols, out, stats, srows, false);
}

/* The way out of a transformer in patch token order (proj_out): mode 0 / 4 of sdm_op_gemm_p3 where row t of image n of x is TOKEN t (sdm_common.h), and `out` / `res`
 * are pixel-order rows [N][H][W][O] - the result of token t lands at (and its residual comes from) the token's pixel.  patch_tokens = 0: the plain launch. */
int sdm_op_gemm_p3_tokens(sdm_ctx* e, const float* x, int N, int H, int W, int K, const float* w, const float* bias, int O, int mode, const float* res,
                          int patch_tokens, float* out, float* stats, int* srows) {
  if (mode != 0 && mode != 4) return SDM_ERR_INVALID;
  return gemm_p3_hook(e, x, N, H, W, K, w, bias, O, mode, res, nullptr, nullptr, 0.0f, -1, out, stats, srows, patch_tokens != 0);
}

/* The way in (GroupNorm -> the P3 operand planes of proj_in): x fp32 [N][H][W][C] -> planes (ceil(N*H*W / 32) * 32 * C * 3 bytes each: fp16 hi plane, then the xl
 * plane) in row-major order (planes_rows) and / or with row t of an image = token t (planes_tokens); either may be NULL.  Both come from ONE statistics pass: the
 * statistics kernel adds with atomics, so two passes may differ in the last bit. */
int sdm_op_groupnorm_p3(sdm_ctx* e, const float* x, int N, int H, int W, int C, int groups, const float* gamma, const float* beta, float eps, int silu,
                        void* planes_rows, void* planes_tokens) {
  if (e) dev_use(e->device);
  if (!e || !x || (!planes_rows && !planes_tokens) || C % 32) return SDM_ERR_INVALID;
  if (planes_tokens && !sdm_patch_tokens_ok(H, W)) SDM_FAIL(e, SDM_ERR_INVALID, "sdm_op_groupnorm_p3: %dx%d does not take the patch token order", H, W);
  return run_two_pass(e, [&]() -> int {
    T scratch; float* scale; float* shift;
    TRY(gn_scale_shift(e, x, nullptr, C, 0, 1, N, H * W, groups, gamma, beta, eps, nullptr, 0, nullptr, 0, false, &scratch, &scale, &shift));
    if (!e->dry) {
      GnSrc s; s.in0 = x; s.in1 = nullptr; s.C0 = C; s.C1 = 0; s.in_f32 = 1; s.HW = H * W;
      const long rows = (long)N * H * W;
      if (planes_rows)
        SDM_LAUNCH(gn_apply_p3_kernel, dim3((unsigned)((rows + 15) / 16)), dim3(256), 0, e->stream, s, (const float*)scale, (const float*)shift, (unsigned char*)planes_rows, silu, rows, 0);
      if (planes_tokens)
        SDM_LAUNCH(gn_apply_p3_kernel, dim3((unsigned)((rows + 15) / 16)), dim3(256), 0, e->stream, s, (const float*)scale, (const float*)shift, (unsigned char*)planes_tokens, silu, rows, W);
    }
    tfree(e, scratch);
    return 0;
  });
}

/* The helper pair of the patch token order as the kernels use it: token_of_pixel[y * W + x] and pixel_of_token[t] (HOST, H * W ints each) of one image.
 * Returns 1 if an H x W latent takes the order (sdm_patch_tokens_ok), else 0 with both maps the identity (row-major), < 0 on bad arguments. */
int sdm_debug_patch_token_map(int H, int W, int32_t* token_of_pixel, int32_t* pixel_of_token) {
  if (H < 1 || W < 1 || !token_of_pixel || !pixel_of_token) return SDM_ERR_INVALID;
  const bool on = sdm_patch_tokens_ok(H, W);
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) token_of_pixel[y * W + x] = on ? (int32_t)sdm_patch_token_of_pixel((unsigned int)y, (unsigned int)x, (unsigned int)W) : y * W + x;
  for (int t = 0; t < H * W; ++t) pixel_of_token[t] = on ? (int32_t)sdm_patch_pixel_of_token((unsigned int)t, (unsigned int)W) : t;
  return on ? 1 : 0;
}

/* Upsample2D (nearest x2 + 3x3 conv, split precision, fp32 NHWC in and out) with the consumer's GroupNorm statistics, as the model's up-sampling layers run
 * it: `out` [N][2H][2W][O], `stats` [N][*srows][O][2] partial {sum, sumsq} rows (at most 8 * ceil((H + 2)(W + 2) / 64) + 4 * ceil(H / 2) * ceil(W / 4) rows per image).  C % 32 == 0 and
 * O % 32 == 0: the phase path (k_gemm.h, UP) where the model would take it (option conv_up_phase: 1 by launch size, 2 always, 0 never). */
int sdm_op_conv_up_stats(sdm_ctx* e, const float* x, int N, int H, int W, int C, const float* w, const float* bias, int O, float* out, float* stats, int* srows) {
  if (e) dev_use(e->device);
  if (!e || !x || !w || !out || !stats || !srows) return SDM_ERR_INVALID;
  if (C % 32 || O % 32) SDM_FAIL(e, SDM_ERR_INVALID, "sdm_op_conv_up_stats: C %% 32 and O %% 32 required");
  TempLayer tl(e);
  TRY(tl.init("op_up", 9, C, O, 0, 1, TempLayer::kDma | TempLayer::kUp, w, bias));
  return run_two_pass(e, [&]() -> int {
    T tin = view(x, N, H, W, C, 1), to = view(out, N, 2 * H, 2 * W, O, 1);
    to.want_stats = true;
    ConvArgs a; a.in0 = &tin; a.out = &to; a.up = 1;
    TRY(op_conv(e, tl.L, a));
    if (!e->dry) {
      SDM_CHECK_DEV(e, dev_memcpy_d2d(stats, to.stats, (size_t)N * to.srows * O * 2 * 4, e->stream));
      *srows = to.srows;
    }
    if (to.sbytes) { tfree_raw(e, to.soff, to.sbytes); to.sbytes = 0; }
    return 0;
  });
}

/* Test hook: `mask` (device, [N][Hin][Win] bytes, class ids 0..4; k_misc.h cmask_*) is the class plane of the input of the NEXT sdm_op_conv_ex / sdm_op_conv_stats call -
 * the conv then leaves the output tiles of constant regions to const_tile_fill_kernel, as the VAE encoder does for the trimap images. */
int sdm_debug_set_input_cmask(sdm_ctx* e, const unsigned char* mask) {
  if (!e) return SDM_ERR_INVALID;
  e->dbg_cmask = mask;
  return SDM_OK;
}

int sdm_op_conv(sdm_ctx* e, const void* in0, const void* in1, int C0, int C1, int in_f32, int N, int Hin, int Win, int up, int stride,
                int pad_mode, int ntaps, const float* w, const float* bias, int O, void* out, int out_f32, const void* res, int res_f32,
                int geglu, float out_scale, int tile_cfg) {
  return sdm_op_conv_ex(e, in0, in1, C0, C1, in_f32, N, Hin, Win, up, stride, pad_mode, ntaps, w, bias, O, out, out_f32, res, res_f32, geglu,
                        out_scale, tile_cfg, 0, nullptr, nullptr, 0.0f, 32, 0);
}

/* ---- test hooks for the exact algebraic folds (SURVEY.md 8a "each needs a fold == unfold CPU test") ----------------------- */

/* Run ONE packed layer of the loaded model (by name, e.g. "unet.down_blocks.0.attentions.0.transformer_blocks.0.attn2.kv_folded",
 * "...attn1.qkv") on an fp32 NHWC input with the layer's padded input channel count; fp32 NHWC output with `Cout` channels. */
int sdm_debug_run_layer(sdm_ctx* e, const char* layer_name, const float* x, int N, int H, int W, float* out, int Cout) {
  if (e) dev_use(e->device);
  if (!e || !layer_name || !x || !out) return SDM_ERR_INVALID;
  if (!e->finalized) SDM_FAIL(e, SDM_ERR_STATE, "weights not finalised");
  const ConvL* L = nullptr;
  for (auto& c : e->convs) if (c.name == layer_name) { L = &c; break; }
  if (!L) SDM_FAIL(e, SDM_ERR_INVALID, "no packed layer named %s", layer_name);
  if (Cout % 4 || Cout > L->Cout_pad) SDM_FAIL(e, SDM_ERR_INVALID, "bad Cout %d for layer %s", Cout, layer_name);
  T tin = view(x, N, H, W, L->Cin_pad, 1), tout = view(out, N, H, W, Cout, 1);
  ConvArgs a; a.in0 = &tin; a.out = &tout; a.cout_valid = Cout;
  int rc = run_two_pass(e, [&]() { return op_conv(e, *L, a); });
  dev_sync(e->stream);
  return rc;
}

/* Folded conv1 bias row (conv1.bias + time_emb_proj(silu(emb)), emb = time_embedding(trans) + bbox_embedding(coords)) of the
 * i-th ResBlock that has a time embedding, for one (is_trans, box) conditioning; out: cout floats on the HOST. */
int sdm_debug_temb_row(sdm_ctx* e, int temb_index, int is_trans, const float* coords4, float* out_host, int cout) {
  if (e) dev_use(e->device);
  if (!e || !out_host || temb_index < 0 || temb_index >= (int)e->tembs.size()) return SDM_ERR_INVALID;
  if (!e->finalized) SDM_FAIL(e, SDM_ERR_STATE, "weights not finalised");
  int32_t it = is_trans;
  TRY(prepare_variants(e, 1, &it, coords4, 4, 0));
  Variant v; v.trans = 1 - is_trans; v.kind = 0; v.c.assign(4, 0.0f);
  const float def[4] = {0.f, 0.f, 1.f, 1.f};
  for (int k = 0; k < 4; ++k) v.c[k] = coords4 ? coords4[k] : def[k];
  int idx = -1;
  for (size_t i = 0; i < e->variants.size(); ++i) if (e->variants[i] == v) idx = (int)i;
  const TembL& t = e->tembs[(size_t)temb_index];
  if (idx < 0 || cout > t.cout) SDM_FAIL(e, SDM_ERR_INVALID, "temb row: variant not found / bad cout");
  SDM_CHECK_DEV(e, dev_memcpy_d2h(out_host, t.table + (size_t)idx * t.cout_pad, (size_t)cout * 4, e->stream));
  SDM_CHECK_DEV(e, dev_sync(e->stream));
  return SDM_OK;
}

/* bench only: ms per launch of the plane-fed GEMM (k_gemm.h) on random operands: M rows, K -> O, epilogue `epi` (0 fp32, 1 GEGLU, 2 q|k|v planes, 3 P3, 4 fp32 +
 * statistics; bit 8: + fp32 residual).  The row tile follows the option gemm_p3_tile. */
float sdm_bench_gemm_p3(sdm_ctx* e, long M, int K, int O, int epi_flags, int iters) {
  if (e) dev_use(e->device);
  if (!e || K % 32 || O % 64) return -1.f;
#ifdef SDM_EMU
  (void)M; (void)epi_flags; (void)iters;
  return -1.f;
#else
  const int epi = epi_flags & 255, resf = (epi_flags >> 8) & 1;
  DevBuf xf, xp, out, resb, st;
  const int Cst = epi == 1 ? O / 2 : O;
  if (xf.alloc((size_t)M * K * 4) || xp.alloc(p3_rows_pad((size_t)M) * K * 3) || out.alloc(p3_rows_pad((size_t)M) * Cst * 4 + 256)) return -2.f;
  if (resf && resb.alloc((size_t)M * Cst * 4)) return -2.f;
  if (epi == 4 && st.alloc(((size_t)(M + 63) / 64 * 2 + 8) * O * 8)) return -2.f;
  SDM_LAUNCH(fill_random_f32_kernel, dim3(4096), dim3(256), 0, e->stream, (float*)xf.p, (long)M * K, 5u, 1.0f);
  SDM_LAUNCH(to_p3_kernel, dim3(4096), dim3(256), 0, e->stream, (const float*)xf.p, (unsigned char*)xp.p, M, K);
  // weights: random fp32 [O][K] -> K16 hi | lo -> W3, as a model layer (packed without the GEGLU interleave, whatever `epi`); zero bias
  TempLayer tl(e);
  {
    DevBuf wf;
    if (wf.alloc((size_t)K * O * 4)) return -2.f;
    SDM_LAUNCH(fill_random_f32_kernel, dim3(2048), dim3(256), 0, e->stream, (float*)wf.p, (long)K * O, 17u, 0.05f);
    if (tl.init("bench", 1, K, O, 0, 1, TempLayer::kW3, (const float*)wf.p, nullptr) != 0) return -2.f;
  }
  if (resf) SDM_LAUNCH(fill_random_f32_kernel, dim3(4096), dim3(256), 0, e->stream, (float*)resb.p, (long)M * Cst, 31u, 1.0f);
  GemmP3Params p;
  memset(&p, 0, sizeof(p));
  p.M = M; p.K = K; p.a_hi = (const half_t*)xp.p; p.a_xl = (const unsigned char*)xp.p + p3_rows_pad((size_t)M) * K * 2;
  p.w = tl.L.w3; p.N = O; p.bias = tl.L.b; p.out = out.p; p.ldo = Cst; p.n_valid = Cst;
  p.out_lo_off = epi == 2 ? (size_t)M * Cst : p3_rows_pad((size_t)M) * Cst * 2; p.lo_cols = (O / 3) * 2;
  if (resf) { p.res = (const float*)resb.p; p.ldr = Cst; }
  if (epi == 4) { p.stats = (float*)st.p; p.rows_per_img = (int)M; }
  p.sa = 127 - 11; p.sb = 127 - tl.L.f8_exp; p.ablate = opt("gemm_p3_ablate");
  const float ms = time_launches(e, iters, [&]() { launch_gemm_p3(p, epi, e->stream); });
  const hipError_t le = hipGetLastError();
  if (le != hipSuccess) { e->err = hipGetErrorString(le); return -3.f; }
  return ms;
#endif
}

/* Bench/ablation helper (not used by the engine): times `iters` launches of one conv with HIP events; returns ms per launch
 * (negative on error).  ablate bits: see ConvParams::ablate. */
float sdm_bench_conv(sdm_ctx* e, int N, int H, int W, int Cin, int Cout, int ntaps, int stride, int in_f32, int tile_cfg, int ablate, int iters) {
  // in_f32: bit 0 = fp32 activations, bit 1 = split-precision kernel (implies fp32), bit 2 = fused GroupNorm+SiLU staging,
  // bit 3 = producer / consumer form of the split-precision DMA kernel
  const int split = (in_f32 >> 1) & 1, gnf = (in_f32 >> 2) & 1, pcf = (in_f32 >> 3) & 1, f8f = (in_f32 >> 4) & 1;      // bit 4: fp8-residual kernel
  // bits 5-7: what the engine's ResBlock convs do in the default precision - fp32 output, fp32 residual, GroupNorm statistics of the consumer
  const int of32 = (in_f32 >> 5) & 1, resf = (in_f32 >> 6) & 1, statf = (in_f32 >> 7) & 1;
  in_f32 = (in_f32 & 1) | split;
  if (e) dev_use(e->device);
  if (!e) return -1.f;
#ifdef SDM_EMU
  return -1.f;
#else
  ConvL L;
  L.name = "bench"; L.ntaps = ntaps; L.I = Cin; L.O = Cout; L.Cin_pad = rup(Cin, 16); L.Cout_pad = rup(Cout, 32);
  DevBuf wp, bp, in, out, wl, gnt, resb, statb, wdm, wsb;
  const int Ho = stride == 2 ? H / 2 : H, Wo = stride == 2 ? W / 2 : W;
  const size_t wbytes = (size_t)L.Cin_pad * ntaps * L.Cout_pad * 2, inb = (size_t)N * H * W * L.Cin_pad * (in_f32 ? 4 : 2),
               outb = (size_t)N * Ho * Wo * L.Cout_pad * (of32 ? 4 : 2);
  if (wp.alloc(wbytes) || bp.alloc((size_t)L.Cout_pad * 4) || in.alloc(inb) || out.alloc(outb)) return -2.f;
  if (resf) {
    if (resb.alloc((size_t)N * Ho * Wo * L.Cout_pad * 4)) return -2.f;
    SDM_LAUNCH(fill_random_f32_kernel, dim3(4096), dim3(256), 0, e->stream, (float*)resb.p, (long)N * Ho * Wo * L.Cout_pad, 31u, 1.0f);
  }
  if (statf && statb.alloc((size_t)N * (sdm_cdiv(Ho, 4) * sdm_cdiv(Wo, 8) * 4 + 64) * L.Cout_pad * 8)) return -2.f;      // enough partial rows for every tile cfg
  if (split) { if (wl.alloc(wbytes)) return -2.f; SDM_LAUNCH(fill_random_f16_kernel, dim3(2048), dim3(256), 0, e->stream, (half_t*)wl.p, (long)(wbytes / 2), 19u, 0.0001f); }
  if (gnf) {      // scale = 1, shift = 0 table [N][Cin] x 2
    if (gnt.alloc((size_t)N * L.Cin_pad * 8)) return -2.f;
    SDM_LAUNCH(fill_random_f32_kernel, dim3(64), dim3(256), 0, e->stream, (float*)gnt.p, (long)N * L.Cin_pad * 2, 23u, 1.0f);
  }
  dev_memset(bp.p, 0, (size_t)L.Cout_pad * 4, e->stream);
  SDM_LAUNCH(fill_random_f16_kernel, dim3(2048), dim3(256), 0, e->stream, (half_t*)wp.p, (long)(wbytes / 2), 17u, 0.05f);
  if (in_f32) SDM_LAUNCH(fill_random_f32_kernel, dim3(4096), dim3(256), 0, e->stream, (float*)in.p, (long)(inb / 4), 5u, 1.0f);
  else SDM_LAUNCH(fill_random_f16_kernel, dim3(4096), dim3(256), 0, e->stream, (half_t*)in.p, (long)(inb / 2), 5u, 1.0f);
  L.w = (half_t*)wp.p; L.b = (float*)bp.p;
  ConvParams p;
  memset(&p, 0, sizeof(p));
  p.in0 = in.p; p.C0 = L.Cin_pad; p.in_f32 = in_f32; p.N = N; p.Hin = H; p.Win = W; p.Hout = Ho; p.Wout = Wo; p.pad_t = p.pad_l = 1;
  p.M = (long)N * Ho * Wo; p.w = L.w; p.bias = L.b; p.Cout_pad = L.Cout_pad; p.out = out.p; p.Cout_store = L.Cout_pad; p.Cout_valid = L.Cout_pad;
  p.out_scale = 1.f; p.ablate = ablate & 255; p.acc_scale = split ? ldexpf(1.0f, -kSplitWeightExp) : 1.f;
  p.out_f32 = of32; p.epi_mode = conv_epi_mode(); p.xtile = conv_xtile_enabled() ? 1 : 0;
  if (resf) { p.res = resb.p; p.res_f32 = 1; p.res_C = L.Cout_pad; }
  if (statf) p.stats = (float*)statb.p;
  const bool bench_dma_off = opt("conv_dma") == 0;
  if (!bench_dma_off && ntaps == 9 && stride == 1 && L.Cout_pad >= 128) {
    const size_t nb = wbytes * (split ? 2 : 1);
    if (wdm.alloc(nb)) return -2.f;
    SDM_LAUNCH(fill_random_f16_kernel, dim3(2048), dim3(256), 0, e->stream, (half_t*)wdm.p, (long)(nb / 2), 29u, 0.05f);
    p.w_dma = (const half_t*)wdm.p;
  }
  if (split) p.w_lo = (const half_t*)wl.p;
  p.pc = (split && p.w_dma && pcf) ? 1 : 0;
  if (split && p.w_dma && f8f && L.Cin_pad % 32 == 0) { p.f8 = 1; p.f8_sa = 127 - 11; p.f8_sb = 127 - kSplitWeightExp; p.acc_scale = 1.f; }
  if (split && ntaps == 1 && f8f && L.Cin_pad % 32 == 0 && L.Cout_pad >= 128) {      // 1x1 GEMM on the fp8-residual kernel (tile cfg 4)
    if (wdm.alloc(wbytes * 2)) return -2.f;
    SDM_LAUNCH(fill_random_f16_kernel, dim3(2048), dim3(256), 0, e->stream, (half_t*)wdm.p, (long)wbytes, 29u, 0.05f);
    p.w_dma = (const half_t*)wdm.p; p.f8 = 1; p.f8_sa = 127 - 11; p.f8_sb = 127 - kSplitWeightExp; p.acc_scale = 1.f;
  }
  if (gnf) { p.gn_scale = (const float*)gnt.p; p.gn_shift = (const float*)gnt.p + (size_t)N * L.Cin_pad; p.gn_silu = 1; }
  int cfg = tile_cfg >= 0 ? tile_cfg : conv_pick_cfg(ntaps, stride, p);
  // split-K as the engine would run it (option conv_splitk: -1 by shape, n forced); the partial sums + the reduce kernel are inside the timed loop
  int ksplit = 1;
  if (!(p.w_dma && ((ntaps == 9 && stride == 1 && cfg == 0) || (ntaps == 1 && cfg == 4)))) ksplit = conv_pick_ksplit(ntaps, stride, cfg, p);      // register-staged kernels only
  if (ksplit > 1 && wsb.alloc((size_t)ksplit * p.M * p.Cout_pad * 4)) return -2.f;
  if (ksplit > 1) fprintf(stderr, "[bench_conv] split-K %d\n", ksplit);
  auto run = [&](const ConvParams& pp) { if (ksplit > 1) launch_conv_splitk(ntaps, stride, cfg, pp, ksplit, (float*)wsb.p, e->stream); else launch_conv(ntaps, stride, cfg, pp, e->stream); };
  if (ablate & 256) {      // one traced launch of the F8 3x3 kernel (-DSDM_CONV_TRACE builds): the LDS-parked shader-clock stamps of the first 16 blocks -> stderr
    DevBuf tr;
    const size_t tb = (size_t)16 * 2 * 384 * 4;
    if (tr.alloc(tb) == 0) {
      dev_memset(tr.p, 0, tb, e->stream);
      ConvParams pt = p; pt.trace = (unsigned int*)tr.p; pt.ablate = ablate & 255; pt.trace_skip = (ablate >> 9) & 7; pt.trace_b0 = ((ablate >> 12) & 0xFF) * 256;
      launch_conv(ntaps, stride, cfg, pt, e->stream);
      std::vector<unsigned int> h(tb / 4);
      (void)dev_memcpy_d2h(h.data(), tr.p, tb, e->stream);
      (void)dev_sync(e->stream);
      for (int b = 0; b < 16; ++b)
        for (int r = 0; r < 2; ++r) {
          const unsigned int* ev = &h[((size_t)b * 2 + r) * 384];
          const int n = (int)ev[383] < 383 ? (int)ev[383] : 383;
          if (!n) continue;
          fprintf(stderr, "[trace] block %d %s n=%d:", pt.trace_b0 + b, r ? "producer" : "consumer", n);
          for (int i = 0; i < n; ++i) fprintf(stderr, " %u", ev[i]);
          fprintf(stderr, "\n");
        }
    }
    p.ablate = ablate & 255;
  }
  return time_launches(e, iters, [&]() { run(p); });
#endif
}

/* Bench/ablation helper for the d=64 attention kernel (not used by the engine). */
float sdm_bench_attn(sdm_ctx* e, int B, int heads, int Lq, int Lk, int qt, int ablate, int iters) {
  if (e) dev_use(e->device);
  if (!e) return -1.f;
#ifdef SDM_EMU
  return -1.f;
#else
  if (qt & 64) {      // bit 64: the d = 512 single-head kernel (VAE mid-block), ablate = its compile-time ABL mask; bit 256: its ping-pong form (bit 32: without s_setprio)
    const int ldvt5 = rup(Lk, 64);
    DevBuf q5, k5, v5, o5;
    if (q5.alloc((size_t)B * Lq * 512 * 2) || k5.alloc((size_t)B * Lk * 512 * 2) || v5.alloc((size_t)B * 512 * ldvt5 * 2) || o5.alloc((size_t)B * Lq * 512 * 4)) return -2.f;
    SDM_LAUNCH(fill_random_f16_kernel, dim3(4096), dim3(256), 0, e->stream, (half_t*)q5.p, (long)B * Lq * 512, 3u, 0.3f);
    SDM_LAUNCH(fill_random_f16_kernel, dim3(4096), dim3(256), 0, e->stream, (half_t*)k5.p, (long)B * Lk * 512, 7u, 0.3f);
    SDM_LAUNCH(fill_random_f16_kernel, dim3(4096), dim3(256), 0, e->stream, (half_t*)v5.p, (long)B * 512 * ldvt5, 11u, 1.0f);
    AttnParams p5;
    memset(&p5, 0, sizeof(p5));
    p5.q = (const half_t*)q5.p; p5.q_bs = (long)Lq * 512; p5.ldq = 512; p5.k = (const half_t*)k5.p; p5.k_bs = (long)Lk * 512; p5.ldk = 512;
    p5.vt = (const half_t*)v5.p; p5.vt_hs = (long)512 * ldvt5; p5.vt_bs = p5.vt_hs; p5.ldvt = ldvt5; p5.o = (half_t*)o5.p; p5.o_bs = (long)Lq * 512; p5.ldo = 512; p5.o_f32 = 1;
    p5.Lq = Lq; p5.Lk = Lk; p5.scale_log2e = 0.0441941738f * SDM_LOG2E;
    p5.batch = B; p5.heads = 1; p5.nq_blocks = sdm_cdiv(Lq, 128); p5.q_chunks = 8;
    const unsigned nb5 = (unsigned)(B * p5.q_chunks * sdm_cdiv(p5.nq_blocks, p5.q_chunks));
    if (qt & 256) {
      p5.pp_flags = (qt & 32) ? 0 : 1;
      return time_launches(e, iters, [&]() {
#define SDM_D512PP_ABL(A) case A: { auto kp = attn_d512_pp_kernel<A>; SDM_SET_SMEM(kp, ATTN512P_SMEM); SDM_LAUNCH(kp, dim3(nb5), dim3(512), ATTN512P_SMEM, e->stream, p5); } break;
        switch (ablate) { SDM_D512PP_ABL(0) SDM_D512PP_ABL(1) SDM_D512PP_ABL(6) SDM_D512PP_ABL(7) SDM_D512PP_ABL(8) SDM_D512PP_ABL(32) SDM_D512PP_ABL(40) SDM_D512PP_ABL(41) default: break; }
#undef SDM_D512PP_ABL
      });
    }
    return time_launches(e, iters, [&]() {
#define SDM_D512_ABL(A) case A: { auto kp = attn_d512_kernel<A>; SDM_SET_SMEM(kp, ATTN512P_SMEM); SDM_LAUNCH(kp, dim3(nb5), dim3(512), ATTN512P_SMEM, e->stream, p5); } break;
      switch (ablate) { SDM_D512_ABL(0) SDM_D512_ABL(1) SDM_D512_ABL(6) SDM_D512_ABL(7) SDM_D512_ABL(8) SDM_D512_ABL(32) SDM_D512_ABL(40) SDM_D512_ABL(41) default: break; }
#undef SDM_D512_ABL
    });
  }
  const int C = heads * 64, ldvt = rup(Lk, 64);
  const int prec = (qt & 2) ? 1 : 0, nw8 = (qt & 4) ? 1 : 0;          // qt bits: 2 = split-precision variant (hi | lo planes, fp32 output), 4 = 8-wave blocks
  DevBuf q, k, vt, o;
  if (q.alloc((size_t)B * Lq * C * 2 * (1 + prec)) || k.alloc((size_t)B * Lk * C * 2 * (1 + prec)) ||
      vt.alloc((size_t)B * heads * 64 * ldvt * 2 * (1 + prec)) || o.alloc((size_t)B * Lq * C * (prec ? 4 : 2) + 4096)) return -2.f;
  if (prec) {
    SDM_LAUNCH(fill_random_f16_kernel, dim3(4096), dim3(256), 0, e->stream, (half_t*)q.p + (size_t)B * Lq * C, (long)B * Lq * C, 13u, 0.0003f);
    SDM_LAUNCH(fill_random_f16_kernel, dim3(4096), dim3(256), 0, e->stream, (half_t*)k.p + (size_t)B * Lk * C, (long)B * Lk * C, 17u, 0.0003f);
    SDM_LAUNCH(fill_random_f16_kernel, dim3(4096), dim3(256), 0, e->stream, (half_t*)vt.p + (size_t)B * heads * 64 * ldvt, (long)B * heads * 64 * ldvt, 19u, 0.0003f);
  }
  if (prec && (qt & 16)) {      // pair planes: random fp16 bit patterns would hold e5m2 NaNs; zero residual pairs time the same instructions
    (void)hipMemsetAsync((half_t*)q.p + (size_t)B * Lq * C, 0, (size_t)B * Lq * C * 2, (hipStream_t)e->stream);
    (void)hipMemsetAsync((half_t*)k.p + (size_t)B * Lk * C, 0, (size_t)B * Lk * C * 2, (hipStream_t)e->stream);
  }
  SDM_LAUNCH(fill_random_f16_kernel, dim3(4096), dim3(256), 0, e->stream, (half_t*)q.p, (long)B * Lq * C, 3u, 1.0f);
  SDM_LAUNCH(fill_random_f16_kernel, dim3(4096), dim3(256), 0, e->stream, (half_t*)k.p, (long)B * Lk * C, 7u, 1.0f);
  SDM_LAUNCH(fill_random_f16_kernel, dim3(4096), dim3(256), 0, e->stream, (half_t*)vt.p, (long)B * heads * 64 * ldvt, 11u, 1.0f);
  AttnParams p;
  memset(&p, 0, sizeof(p));
  p.q = (const half_t*)q.p; p.q_bs = (long)Lq * C; p.ldq = C; p.k = (const half_t*)k.p; p.k_bs = (long)Lk * C; p.ldk = C;
  p.k_hs = 64;
  p.vt = (const half_t*)vt.p; p.vt_hs = (long)64 * ldvt; p.vt_bs = heads * p.vt_hs; p.ldvt = ldvt; p.o = (half_t*)o.p; p.o_bs = (long)Lq * C; p.ldo = C;
  p.Lq = Lq; p.Lk = Lk; p.scale_log2e = 0.125f * SDM_LOG2E; p.ablate = ablate;
  if (prec) { p.q_lo = (long)B * Lq * C; p.k_lo = (long)B * Lk * C; p.vt_lo = (long)B * p.vt_bs; p.o_f32 = 1; }
  p.batch = B; p.heads = heads; p.nq_blocks = sdm_cdiv(Lq, nw8 ? 256 : 128); p.q_chunks = 8;
  const unsigned nblk = (unsigned)(B * heads * p.q_chunks * sdm_cdiv(p.nq_blocks, p.q_chunks));
  const float ms = time_launches(e, iters, [&]() {
    if (qt & 16) {      // bit 16: the ping-pong kernel (pair planes as the engine's self- and cross-attentions), ablate = its compile-time ABL mask
      p.pp_flags = (qt & 32) ? 0 : 1;
      p.part_ml = (float*)((unsigned char*)o.p + (size_t)B * Lq * C * 4);      // (ablate 64: the segment trace lands behind the output)
      if (qt & 128) p.pp_flags |= 2;
#define SDM_PP_ABL(A) case A: { auto kp = attn_d64_pp_kernel<A, 0, 0>; SDM_SET_SMEM(kp, 160 * 1024); SDM_LAUNCH(kp, dim3(nblk), dim3(512), ATTN64PP_SMEM + 4096, e->stream, p); } break;
#define SDM_PP_DS(A, S, V) case V: { auto kp = attn_d64_pp_kernel<A, 0, 0, 0, S, 0>; SDM_SET_SMEM(kp, 160 * 1024); SDM_LAUNCH(kp, dim3(nblk), dim3(512), ATTN64PP_SMEM + 4096, e->stream, p); } break;
#define SDM_PP_KE(K, V) case V: { auto kp = attn_d64_pp_kernel<0, 0, 0, K, 1, 0>; SDM_SET_SMEM(kp, 160 * 1024); SDM_LAUNCH(kp, dim3(nblk), dim3(512), ATTN64PP_SMEM, e->stream, p); } break;
      switch (ablate) { SDM_PP_ABL(0) SDM_PP_ABL(1) SDM_PP_ABL(6) SDM_PP_ABL(7) SDM_PP_ABL(8) SDM_PP_ABL(32) SDM_PP_ABL(56) SDM_PP_ABL(63)
                        SDM_PP_KE(-1, 100) SDM_PP_KE(2, 101) SDM_PP_KE(1, 102) SDM_PP_ABL(64)
                        SDM_PP_DS(0, 0, 110) SDM_PP_DS(0, 1, 111) SDM_PP_DS(0, 2, 112) SDM_PP_DS(0, 3, 113) SDM_PP_DS(64, 0, 114) SDM_PP_DS(64, 2, 116) SDM_PP_DS(64, 3, 117) default: break; }      // 100-102: the other fragment / DMA placements (KE), no ablation
#undef SDM_PP_ABL
#undef SDM_PP_KE
#undef SDM_PP_DS
    }
    else if (prec && (qt & 8) && nw8) { auto kp = attn_d64_kernel<1, 2, 8>; SDM_SET_SMEM(kp, 160 * 1024); SDM_LAUNCH(kp, dim3(nblk), dim3(512), ATTN64P_SMEM, e->stream, p); }      // bit 8: P.V on plain fp16
    else if (prec && (qt & 8)) { auto kp = attn_d64_kernel<1, 2, 4>; SDM_SET_SMEM(kp, 160 * 1024); SDM_LAUNCH(kp, dim3(nblk), dim3(256), ATTN64P_SMEM, e->stream, p); }
    else if (prec && nw8) { auto kp = attn_d64_kernel<1, 1, 8>; SDM_SET_SMEM(kp, 160 * 1024); SDM_LAUNCH(kp, dim3(nblk), dim3(512), ATTN64P_SMEM, e->stream, p); }
    else if (prec) { auto kp = attn_d64_kernel<1, 1, 4>; SDM_SET_SMEM(kp, 160 * 1024); SDM_LAUNCH(kp, dim3(nblk), dim3(256), ATTN64P_SMEM, e->stream, p); }
    else if (nw8) { auto kf = attn_d64_kernel<1, 0, 8>; SDM_SET_SMEM(kf, 160 * 1024); SDM_LAUNCH(kf, dim3(nblk), dim3(512), ATTN64P_SMEM, e->stream, p); }
    else { SDM_LAUNCH((attn_d64_kernel<1, 0, 4>), dim3(nblk), dim3(256), ATTN64_SMEM, e->stream, p); }
  });
  if ((qt & 16) && (ablate == 64 || (ablate >= 114 && ablate <= 117))) {      // segment stamps of waves 0 (half A) and 4 (half B) of block 0: averages over tiles 4 .. 51 of the last launch
    std::vector<unsigned long long> tr(2 * 8 * 28);
    (void)hipMemcpy(tr.data(), (unsigned char*)o.p + (size_t)B * Lq * C * 4, tr.size() * 8, hipMemcpyDeviceToHost);
    for (int g = 0; g < 2; ++g) {
      double dm = 0, sm = 0, vr = 0, wa = 0, mx = 0, wb = 0; int n = 0;
      for (int t = 5; t < 27; ++t) {
        const unsigned long long* c = &tr[(size_t)g * 224 + (size_t)t * 8];
        const unsigned long long prev3 = tr[(size_t)g * 224 + (size_t)(t - 1) * 8 + 3];
        dm += (double)(c[4] - prev3); sm += (double)(c[5] - c[4]); vr += (double)(c[0] - c[5]); wa += (double)(c[1] - c[0]); mx += (double)(c[2] - c[1]); wb += (double)(c[3] - c[2]); ++n;
      }
      fprintf(stderr, "[attn_pp trace] wave %d: DMA issue %.0f | softmax VALU %.0f | V^T reads + lgkmcnt(0) %.0f | wait at barrier %.0f | matrix segment %.0f | wait at barrier %.0f  (cycles per tile, mean of %d tiles; each stamp costs an s_memtime round trip)\n",
              g * 4, dm / n, sm / n, vr / n, wa / n, mx / n, wb / n, n);
    }
  }
  return ms;
#endif
}

int sdm_op_groupnorm(sdm_ctx* e, const void* in0, const void* in1, int C0, int C1, int in_f32, int N, int HW, int groups, const float* gamma,
                     const float* beta, float eps, int silu, void* out) {
  if (e) dev_use(e->device);
  if (!e || !in0 || !out) return SDM_ERR_INVALID;
  return run_two_pass(e, [&]() { return op_groupnorm_raw(e, in0, in1, C0, C1, in_f32, N, HW, groups, gamma, beta, eps, silu, out, 0); });
}

int sdm_op_layernorm(sdm_ctx* e, const void* x, int in_f32, long rows, int C, const float* gamma, const float* beta, float eps, void* out) {
  if (e) dev_use(e->device);
  if (!e || !x || !out) return SDM_ERR_INVALID;
  if (C % 64 || C > 64 * SDM_LN_MAXV) SDM_FAIL(e, SDM_ERR_INVALID, "layernorm: unsupported C %d", C);
  SDM_LAUNCH(layernorm_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, e->stream, x, in_f32, gamma, beta, out, 0, rows, C, eps);
  SDM_CHECK_DEV(e, dev_sync(e->stream));
  return 0;
}

int sdm_op_attention(sdm_ctx* e, const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, const float* bias, int B, int heads,
                     int Lq, int Lk, int D, void* out, int ldo) {
  if (e) dev_use(e->device);
  if (!e || !q || !k || !v || !out) return SDM_ERR_INVALID;
  return run_two_pass(e, [&]() {
    T b2 = talloc(e, B, 1, 1, Lk, 1);
    AttnPrec ap; ap.has_bias = bias != nullptr;
    if (bias && !e->dry) {
      // natural-log bias (reference domain) -> log2 domain used by the kernel
      SDM_LAUNCH(scale_copy_kernel, dim3(sdm_cdiv(B * Lk, 256)), dim3(256), 0, e->stream, bias, (float*)b2.p, (long)B * Lk, SDM_LOG2E);
    }
    int rc = op_attention_raw(e, (const half_t*)q, ldq, (const half_t*)k, ldk, (const half_t*)v, ldv, bias ? (const float*)b2.p : nullptr,
                              B, heads, Lq, Lk, D, (half_t*)out, ldo, false, nullptr, ap);
    tfree(e, b2);
    return rc;
  });
}

/* sdm_op_attention with an fp32 result (out_f32 != 0: `out` is fp32 [B][Lq][heads*D], ldo in elements) - the d = 512 core as the precise-mode VAE runs it.  Test hook. */
int sdm_op_attention_ex(sdm_ctx* e, const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, int B, int heads, int Lq, int Lk, int D, int out_f32,
                        void* out, int ldo) {
  if (e) dev_use(e->device);
  if (!e || !q || !k || !v || !out) return SDM_ERR_INVALID;
  if (out_f32 && D != 512) SDM_FAIL(e, SDM_ERR_INVALID, "sdm_op_attention_ex: fp32 output of fp16 operands exists for head dim 512 only");
  return run_two_pass(e, [&]() {
    AttnPrec ap; ap.out_f32 = out_f32 ? 1 : 0;
    return op_attention_raw(e, (const half_t*)q, ldq, (const half_t*)k, ldk, (const half_t*)v, ldv, nullptr, B, heads, Lq, Lk, D, out, ldo, false, nullptr, ap);
  });
}

/* Split-precision d = 64 attention cores as the default precision runs them.  q [B,Lq,heads*64], k / v [B,Lk,heads*64]: contiguous fp32
 * DEVICE tensors.  They are first turned into the operand planes the producing GEMMs write in the engine (split_planes_kernel: fp16 hi plane
 * + fp16 lo plane, or + e5m2 pair plane when the Q.K^T residual terms run on fp8 MFMAs - the default; the option attn_f8 = 0 selects the former),
 * with the logit scale d^-1/2 * log2(e) applied to Q as the engine's to_q weights do; fp32 output [B,Lq,heads*64].  Test hook. */
int sdm_op_attention_split(sdm_ctx* e, const float* q, const float* k, const float* v, const float* bias, int B, int heads, int Lq, int Lk, float* out) {
  return sdm_op_attention_split_ex(e, q, k, v, bias, nullptr, B, heads, Lq, Lk, 0, out, nullptr);
}

int sdm_op_attention_split_ex(sdm_ctx* e, const float* q, const float* k, const float* v, const float* bias, const int* tiles, int B, int heads, int Lq,
                              int Lk, int out_p3, float* out, void* planes) {
  if (e) dev_use(e->device);
  if (!e || !q || !k || !v || !out) return SDM_ERR_INVALID;
  if (out_p3 < 0 || out_p3 > 2 || (tiles && !bias)) SDM_FAIL(e, SDM_ERR_INVALID, "sdm_op_attention_split_ex: out_p3 0..2; a tile list needs the bias");
  const int C = heads * 64;
  const int mode = (attn_f8_enabled() && !opt("attn_pv_split")) ? 3 : 2;
  return run_two_pass(e, [&]() -> int {
    T b2 = talloc(e, B, 1, 1, Lk, 1);
    T qp = talloc(e, B, 1, Lq, C, mode), kp = talloc(e, B, 1, Lk, C, mode), vp = talloc(e, B, 1, Lk, C, mode);
    const long nq = (long)B * Lq * C, nk = (long)B * Lk * C;
    if (!e->dry) {
      if (bias) SDM_LAUNCH(scale_copy_kernel, dim3(sdm_cdiv(B * Lk, 256)), dim3(256), 0, e->stream, bias, (float*)b2.p, (long)B * Lk, SDM_LOG2E);
      SDM_LAUNCH(split_planes_kernel, dim3((unsigned)((nq / 4 + 255) / 256)), dim3(256), 0, e->stream, q, (half_t*)qp.p, (half_t*)qp.p + nq, nq, 0.125f * SDM_LOG2E, mode);
      SDM_LAUNCH(split_planes_kernel, dim3((unsigned)((nk / 4 + 255) / 256)), dim3(256), 0, e->stream, k, (half_t*)kp.p, (half_t*)kp.p + nk, nk, 1.0f, mode);
      SDM_LAUNCH(split_planes_kernel, dim3((unsigned)((nk / 4 + 255) / 256)), dim3(256), 0, e->stream, v, (half_t*)vp.p, (half_t*)vp.p + nk, nk, 1.0f, 2);
    }
    // out_p3 = 1: the planes written by the kernels (the engine's default); 2: an fp32 result, then to_p3_kernel
    T to, pl;
    if (out_p3) to = talloc(e, B, 1, Lq, C, out_p3 == 1 ? kFmtP3 : 1);
    AttnPrec ap; ap.prec = mode - 1; ap.q_lo = nq; ap.k_lo = nk; ap.v_lo = nk; ap.out_f32 = 1; ap.out_p3 = out_p3 == 1;
    ap.has_bias = bias != nullptr; ap.has_tiles = tiles != nullptr;
    TRY(op_attention_raw(e, (const half_t*)qp.p, C, (const half_t*)kp.p, C, (const half_t*)vp.p, C, bias ? (const float*)b2.p : nullptr, B, heads, Lq, Lk, 64,
                         out_p3 ? to.p : (void*)out, C, true, tiles, ap));
    if (out_p3 == 2) TRY(op_to_p3(e, to, &pl));
    const T& p3 = out_p3 == 2 ? pl : to;
    if (out_p3 && !e->dry) {
      SDM_LAUNCH(from_p3_kernel, dim3((unsigned)std::min<long>(((long)B * Lq * C + 255) / 256, 1 << 20)), dim3(256), 0, e->stream, (const unsigned char*)p3.p, out,
                 (long)B * Lq, C);
      if (planes) SDM_CHECK_DEV(e, dev_memcpy_d2d(planes, p3.p, p3_rows_pad((size_t)B * Lq) * C * 3, e->stream));
    }
    if (out_p3 == 2) tfree(e, pl);
    if (out_p3) tfree(e, to);
    tfree(e, vp); tfree(e, kp); tfree(e, qp); tfree(e, b2);
    return 0;
  });
}

/* The shared key / value operand of the cross-attentions (cross_patch_planes_kernel) of a U-Net input tensor uin fp32 [B][H][W][16] (DEVICE; the trimap latent
 * at channels 4..7): k_hi [B][H*W][64] fp16, k_pair the same number of bytes (the e5m2 pair plane), vt [B][64][rup(H*W, 64)] fp16.  Test hook. */
int sdm_op_cross_patch_planes(sdm_ctx* e, const float* uin, int B, int H, int W, void* k_hi, void* k_pair, void* vt) {
  return sdm_op_cross_patch_planes_ex(e, uin, B, H, W, k_hi, k_pair, vt, 0);
}
/* ... ones_rows != 0: with 1.0 in V^T rows 59 and 63 for the key columns < H*W, as the engine builds the operand under the option cross_narrow.  Test hook. */
int sdm_op_cross_patch_planes_ex(sdm_ctx* e, const float* uin, int B, int H, int W, void* k_hi, void* k_pair, void* vt, int ones_rows) {
  if (e) dev_use(e->device);
  if (!e || !uin || !k_hi || !k_pair || !vt || B < 1 || H < 1 || W < 1) return SDM_ERR_INVALID;
  const int Lk = H * W, ldvt = rup(Lk, 64);
  const long nthr = std::max((long)B * Lk * 8, (long)B * 64 * (ldvt / 8));
  count_kernel("cross_patch_planes");
  SDM_LAUNCH(cross_patch_planes_kernel, dim3((unsigned)((nthr + 255) / 256), 2, 1), dim3(256), 0, e->stream, uin, B, H, W, (half_t*)k_hi, (half_t*)k_pair, (half_t*)vt, ldvt, ones_rows ? 1 : 0);
  SDM_CHECK_DEV(e, dev_sync(e->stream));
  return 0;
}

/* sdm_op_attention_split on ONE key / value operand for every head (AttnPrec::shared_kv: head stride 0 for K and V^T, no V^T scratch, no transpose_v launch
 * inside the operator): q fp32 [B,Lq,heads*64], ks / vs fp32 [B,Lk,64]; q_prescaled != 0: the logit scale is in q already; fp32 output [B,Lq,heads*64].
 * Needs the fp8-pair plane format (options attn_f8 = 1, attn_pv_split = 0).  Test hook. */
int sdm_op_attention_shared(sdm_ctx* e, const float* q, const float* ks, const float* vs, int B, int heads, int Lq, int Lk, int q_prescaled, float* out) {
  if (e) dev_use(e->device);
  if (!e || !q || !ks || !vs || !out) return SDM_ERR_INVALID;
  if (!attn_f8_enabled() || opt("attn_pv_split")) SDM_FAIL(e, SDM_ERR_INVALID, "sdm_op_attention_shared: the fp8-pair plane format only");
  const int C = heads * 64, ldvt = rup(Lk, 64);
  return run_two_pass(e, [&]() -> int {
    T qp = talloc(e, B, 1, Lq, C, 3), kp = talloc(e, B, 1, Lk, 64, 3), vp = talloc(e, B, 1, Lk, 64, 2), vt = talloc(e, B, 1, 64, ldvt, 0);
    const long nq = (long)B * Lq * C, nk = (long)B * Lk * 64;
    if (!e->dry) {
      SDM_LAUNCH(split_planes_kernel, dim3((unsigned)((nq / 4 + 255) / 256)), dim3(256), 0, e->stream, q, (half_t*)qp.p, (half_t*)qp.p + nq, nq,
                 q_prescaled ? 1.0f : 0.125f * SDM_LOG2E, 3);
      SDM_LAUNCH(split_planes_kernel, dim3((unsigned)((nk / 4 + 255) / 256)), dim3(256), 0, e->stream, ks, (half_t*)kp.p, (half_t*)kp.p + nk, nk, 1.0f, 3);
      SDM_LAUNCH(split_planes_kernel, dim3((unsigned)((nk / 4 + 255) / 256)), dim3(256), 0, e->stream, vs, (half_t*)vp.p, (half_t*)vp.p + nk, nk, 1.0f, 2);
      SDM_LAUNCH(transpose_v_kernel, dim3(ldvt / 64, 1, B), dim3(256), 0, e->stream, (const half_t*)vp.p, (long)Lk * 64, 64, (half_t*)vt.p, (long)64 * ldvt,
                 (long)64 * ldvt, ldvt, Lk, 64);
    }
    AttnPrec ap; ap.prec = 2; ap.q_lo = nq; ap.k_lo = nk; ap.out_f32 = 1; ap.shared_kv = true;
    TRY(op_attention_raw(e, (const half_t*)qp.p, C, (const half_t*)kp.p, 64, (const half_t*)vt.p, 64, nullptr, B, heads, Lq, Lk, 64, (void*)out, C, true, nullptr, ap));
    tfree(e, vt); tfree(e, vp); tfree(e, kp); tfree(e, qp);
    return 0;
  });
}

/* The cross-attention of ONE transformer block of the loaded model as the forward runs it under the current options (cross_shared: the shared operand with
 * q_shared / out_shared, or the block's own kv_folded + to_q / to_out.0): block = "unet.down_blocks.0.attentions.0" etc.; x fp32 [B][H][W][C] (DEVICE) is the
 * normalised hidden state (the output of norm2), uin fp32 [B][h][w][16] the U-Net input tensor; out fp32 [B][H][W][C] = to_out(attention), no residual.
 * Needs an engine with fp32 activations and an fp32 stream (the default precision).  Test hook. */
int sdm_debug_cross_attention(sdm_ctx* e, const char* block, const float* x, int B, int H, int W, const float* uin, int h, int w, float* out) {
  if (e) dev_use(e->device);
  if (!e || !block || !x || !uin || !out) return SDM_ERR_INVALID;
  if (!e->finalized) SDM_FAIL(e, SDM_ERR_STATE, "weights not finalised");
  if (!e->act_f32 || e->cfg.stream_f32 != 1) SDM_FAIL(e, SDM_ERR_INVALID, "sdm_debug_cross_attention: fp32 activations and stream expected");
  std::vector<const TfB*> blocks;
  for (auto& v : e->u_down_tf) for (auto& t : v) blocks.push_back(&t);
  blocks.push_back(&e->u_midtf);
  for (auto& v : e->u_up_tf) for (auto& t : v) blocks.push_back(&t);
  const TfB* tb = nullptr;
  for (const TfB* t : blocks) if (e->convs[t->q2].name == std::string(block) + ".transformer_blocks.0.attn2.to_q") tb = t;
  if (!tb) SDM_FAIL(e, SDM_ERR_INVALID, "no transformer block named %s", block);
  const int C = tb->C;
  return run_two_pass(e, [&]() -> int {
    const int pf = unet_attn_plane_fmt(e);
    const bool p3 = transformer_p3(e, *tb, pf), p3a = p3 && (H * W) % 32 == 0 && opt("gemm_p3_attn") != 0;
    const T tu = view(uin, B, h, w, 16, 1), tx = view(x, B, H, W, C, 1);
    CrossPlanes cp;
    TRY(cross_planes_build(e, tu, &cp));
    T n = tx, o;
    if (p3) TRY(op_to_p3(e, tx, &n));
    TRY(cross_attention(e, *tb, n, tu, cp, pf, p3, p3a, nullptr, &o));
    if (!e->dry) SDM_CHECK_DEV(e, dev_memcpy_d2d(out, o.p, (size_t)B * H * W * C * 4, e->stream));
    tfree(e, o);
    cross_planes_free(e, &cp);
    return 0;
  });
}

/* The attention core of a cross-attention on the engine's OWN shared operand, for any number of heads (the tiny architecture has blocks of 1 and 2): q fp32
 * [B][Lq][heads*64] (DEVICE; pre-scaled logits, columns 36..63 of every head zero as q_shared leaves them) attends to the planes that cross_planes_build makes
 * of uin fp32 [B][h][w][16] under the current options (cross_narrow: ones rows and the narrow form) -> the core's fp32 output [B][Lq][heads*64], whose columns
 * 0..35 per head are what out_shared reads.  Test hook. */
int sdm_op_cross_core(sdm_ctx* e, const float* q, const float* uin, int B, int heads, int Lq, int h, int w, float* out) {
  if (e) dev_use(e->device);
  if (!e || !q || !uin || !out || B < 1 || heads < 1 || Lq < 1 || h < 1 || w < 1) return SDM_ERR_INVALID;
  const int C = heads * 64, Lk = h * w;
  return run_two_pass(e, [&]() -> int {
    const T tu = view(uin, B, h, w, 16, 1);
    CrossPlanes cp;
    TRY(cross_planes_build(e, tu, &cp));
    if (!cp.on) SDM_FAIL(e, SDM_ERR_INVALID, "sdm_op_cross_core: the shared operand is off (cross_shared = 0 or another plane format)");
    T qp = talloc(e, B, 1, Lq, C, 3);
    const long nq = (long)B * Lq * C;
    if (!e->dry) SDM_LAUNCH(split_planes_kernel, dim3((unsigned)((nq / 4 + 255) / 256)), dim3(256), 0, e->stream, q, (half_t*)qp.p, (half_t*)qp.p + nq, nq, 1.0f, 3);
    AttnPrec ap; ap.prec = 2; ap.q_lo = nq; ap.k_lo = (long)B * Lk * 64; ap.out_f32 = 1; ap.shared_kv = true; ap.narrow36 = cp.narrow;
    TRY(op_attention_raw(e, (const half_t*)qp.p, C, (const half_t*)cp.k.p, 64, (const half_t*)cp.vt.p, 64, nullptr, B, heads, Lq, Lk, 64, (void*)out, C, true, nullptr, ap));
    tfree(e, qp);
    cross_planes_free(e, &cp);
    return 0;
  });
}

int sdm_debug_attn_plan(int B, int heads, int Lq, int Lk, int D, int prec, int out_f32, int has_bias, int has_tiles, int cus, char* kernel, int cap,
                        int* nsplit) {
  if (B < 1 || heads < 1 || Lq < 1 || Lk < 1 || cus < 1 || prec < 0 || prec > 2 || !(D == 64 || (D == 512 && heads == 1 && !prec))) return SDM_ERR_INVALID;
  OptReadLock opt_lock;
  const AttnPlan pl = attn_plan(B, heads, Lq, Lk, D, prec, out_f32, has_bias != 0, has_tiles != 0, cus);
  if (kernel && cap > 0) snprintf(kernel, (size_t)cap, "%s", kAttnKernels[pl.kernel].counter);
  if (nsplit) *nsplit = pl.nsplit;
  return SDM_OK;
}

int sdm_op_resize_aa(sdm_ctx* e, const float* in, int P, int Hin, int Win, float* out, int Hout, int Wout) {
  if (e) dev_use(e->device);
  if (!e || !in || !out) return SDM_ERR_INVALID;
  SDM_LAUNCH(resize_planes_kernel, dim3((unsigned)(((long)P * Hout * Wout + 255) / 256)), dim3(256), 0, e->stream, in, out, P, Hin, Win, Hout, Wout, 0);
  SDM_CHECK_DEV(e, dev_sync(e->stream));
  return 0;
}

int sdm_op_mask_bias(sdm_ctx* e, const float* plane, int B, int S, int level, float* out) {
  if (e) dev_use(e->device);
  if (!e || !plane || !out) return SDM_ERR_INVALID;
  const int lk = (S / 8) >> level;
  SDM_LAUNCH(mask_bias_kernel, dim3(sdm_cdiv(B * lk * lk, 256)), dim3(256), 0, e->stream, plane, out, B, S, S, level, e->cfg.attn_mask_value, 1.0f, 0);
  SDM_CHECK_DEV(e, dev_sync(e->stream));
  return 0;
}

/* The level's key bias as the U-Net passes it to its self-attentions, on a rectangle: log2 domain, and in patch token order if patch_tokens != 0 and the level's
 * latent takes it (sdm_patch_tokens_ok; otherwise row-major).  Returns 1 / 0 = the order written, < 0 on error. */
int sdm_op_mask_bias_tokens(sdm_ctx* e, const float* plane, int B, int SH, int SW, int level, int patch_tokens, float* out) {
  if (e) dev_use(e->device);
  if (!e || !plane || !out || level < 0 || level > 3) return SDM_ERR_INVALID;
  const int hk = (SH / 8) >> level, wk = (SW / 8) >> level;
  if (hk < 1 || wk < 1) return SDM_ERR_INVALID;
  const int pt = (patch_tokens && sdm_patch_tokens_ok(hk, wk)) ? 1 : 0;
  SDM_LAUNCH(mask_bias_kernel, dim3(sdm_cdiv(B * hk * wk, 256)), dim3(256), 0, e->stream, plane, out, B, SH, SW, level, e->cfg.attn_mask_value, SDM_LOG2E, pt);
  SDM_CHECK_DEV(e, dev_sync(e->stream));
  return pt;
}

/* The list of active 64-key tiles the engine builds from a key bias [B][Lk] (log2 domain): tiles int [B][ceil(Lk / 64) + 1] = count, then ascending tile indices. */
int sdm_op_active_tiles(sdm_ctx* e, const float* bias, int B, int Lk, int32_t* tiles) {
  if (e) dev_use(e->device);
  if (!e || !bias || !tiles || B < 1 || Lk < 1) return SDM_ERR_INVALID;
  const int nt = sdm_cdiv(Lk, 64);
  SDM_LAUNCH(attn_active_tiles_kernel, dim3(B), dim3(256), 0, e->stream, bias, Lk, nt, (int*)tiles, nt + 1, SDM_ATTN_SKIP_MARGIN);
  SDM_CHECK_DEV(e, dev_sync(e->stream));
  return 0;
}

}  // extern "C"
