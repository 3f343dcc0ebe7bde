// sdm_engine.cpp - MI355X-native SDMatte engine: model graph, weight registry/packing, activation arena and
// the product C ABI of include/sdmatte.h (its test hooks and bench helpers: sdm_hooks.h, included at the end).  Compiled with `hipcc -x hip --offload-arch=gfx950` (product), or with
// -DSDM_EMU against tests/emu/hip_emu.h (kernel-debug build used by tests only; never shipped).
//
// The graph executed by run_model() restates SDMatte.forward (/root/reference/src/modeling/SDMatte/
// meta_arch.py:127-261) and CustomUNet.forward (/root/reference/src/utils/replace.py:379-549) over the
// diffusers SD-2.1 blocks they instantiate, re-designed for gfx950:
//   * NHWC activations, fp16 MFMA operands, fp32 accumulation/statistics, fp32 residual stream;
//   * the rgb and trimap VAE encodes run as ONE batch of 2B images (same weights);
//   * q|k|v and cross k|v projections are single fused GEMMs; GEGLU is a GEMM epilogue;
//   * time/opacity/bbox embeddings are constants per (is_trans, coords): computed once on the host and
//     folded into every ResBlock conv1 bias;
//   * the dead CLIP text branch (meta_arch.py:220-234, never consumed: replace.py:414-416) is not built.
#include "sdm_common.h"
#include "k_conv.h"
#include "k_gemm.h"
#include "k_norm.h"
#include "k_attn.h"
#include "k_misc.h"
#include "k_trimap.h"
#include "k_cclabel.h"
#include "k_foreground.h"
#include "k_guided.h"
#include "k_temporal.h"
#include "k_motion.h"
#include "k_defocus.h"
#include "k_plate.h"
#include "k_harmonize.h"
#include "k_key.h"
#include "k_metrics.h"
#include "k_roi.h"
#include "k_canvas.h"
#include "k_boxes.h"
#include "k_tiles.h"
#include "k_distance.h"
#include "../../include/sdmatte.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <atomic>
#include <map>
#include <mutex>
#include <shared_mutex>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

// ------------------------------------------------------------------------------------------------
// device runtime shim
// ------------------------------------------------------------------------------------------------
#ifdef SDM_EMU
#include <chrono>
static int dev_malloc(void** p, size_t n) { *p = aligned_alloc(256, ((n + 255) / 256) * 256 + 256); return *p ? 0 : -1; }
static void dev_free(void* p) { free(p); }
static int dev_memcpy_h2d(void* d, const void* s, size_t n, void*) { memcpy(d, s, n); return 0; }
static int dev_memcpy_d2h(void* d, const void* s, size_t n, void*) { memcpy(d, s, n); return 0; }
static int dev_memcpy_d2d(void* d, const void* s, size_t n, void*) { memcpy(d, s, n); return 0; }
static int dev_memset(void* d, int v, size_t n, void*) { memset(d, v, n); return 0; }
static int dev_sync(void*) { return 0; }
static const char* dev_errstr(int) { return "emu"; }
#define SDM_SET_SMEM(kernel, bytes) ((void)0)
#else
static int dev_malloc(void** p, size_t n) { return (int)hipMalloc(p, n); }
static void dev_free(void* p) { (void)hipFree(p); }
static int dev_memcpy_h2d(void* d, const void* s, size_t n, void* st) { return (int)hipMemcpyAsync(d, s, n, hipMemcpyHostToDevice, (hipStream_t)st); }
static int dev_memcpy_d2h(void* d, const void* s, size_t n, void* st) { return (int)hipMemcpyAsync(d, s, n, hipMemcpyDeviceToHost, (hipStream_t)st); }
static int dev_memcpy_d2d(void* d, const void* s, size_t n, void* st) { return (int)hipMemcpyAsync(d, s, n, hipMemcpyDeviceToDevice, (hipStream_t)st); }
static int dev_memset(void* d, int v, size_t n, void* st) { return (int)hipMemsetAsync(d, v, n, (hipStream_t)st); }
static int dev_sync(void* st) { return (int)hipStreamSynchronize((hipStream_t)st); }
static const char* dev_errstr(int e) { return hipGetErrorString((hipError_t)e); }
// Kernels with more than 48 KB of dynamic LDS need the attribute once PER DEVICE (one process may drive one engine per GPU,
// INTEGRATION.md 3): a bit per device id, set with relaxed atomics (setting it twice is harmless).
#define SDM_SET_SMEM(kernel, bytes)                                                                              \
  do {                                                                                                           \
    if ((bytes) > 48 * 1024) {                                                                                   \
      static std::atomic<unsigned long long> done_{0ull};                                                        \
      int dev_ = 0;                                                                                              \
      (void)hipGetDevice(&dev_);                                                                                 \
      const unsigned long long bit_ = 1ull << (dev_ & 63);                                                       \
      if (!(done_.load(std::memory_order_relaxed) & bit_)) {                                                     \
        const hipError_t r_ = hipFuncSetAttribute((const void*)(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(bytes)); \
        if (r_ != hipSuccess) fprintf(stderr, "[sdmatte] hipFuncSetAttribute(%d bytes of LDS) failed: %s\n", (int)(bytes), hipGetErrorString(r_)); \
        else done_.fetch_or(bit_, std::memory_order_relaxed);                                                    \
      }                                                                                                          \
    }                                                                                                            \
  } while (0)
#endif

static inline int rup(int a, int b) { return ((a + b - 1) / b) * b; }
// every entry point that touches the GPU selects the engine's device first: one process may own one engine per GPU
#ifdef SDM_EMU
static inline void dev_use(int) {}
#else
static inline void dev_use(int device) {
  const hipError_t r = hipSetDevice(device);
  if (r != hipSuccess) fprintf(stderr, "[sdmatte] hipSetDevice(%d) failed: %s\n", device, hipGetErrorString(r));   // the next HIP call of the entry point reports it through its status
}
#endif
static inline size_t rupz(size_t a, size_t b) { return ((a + b - 1) / b) * b; }

// ------------------------------------------------------------------------------------------------
// kernel-selection options.  The product reads NO environment variable on any path: every choice below has ONE default, and the only
// way to change one is the C ABI (sdm_set_option; tests and the A/B tools under tools/ use it).  sdm_kernel_counts reports which
// variants actually ran, so that a test can assert the kernel it meant to check.
// ------------------------------------------------------------------------------------------------
struct OptEntry { const char* name; int value; int def; const char* what; };
static OptEntry g_opts[] = {
  {"conv_f8", 1, 1, "residual terms of the wide split-precision 3x3 convs on fp8 MFMAs (read when a model is built)"},
  {"gemm_f8", 1, 1, "the same for Linear / 1x1 layers with K >= gemm_f8_min_k (read when a model is built)"},
  {"gemm_f8_min_k", 1024, 1024, "smallest K of a GEMM that takes the 8-wave fp8-residual kernel"},
  {"gemm_p3", 1, 1, "transformer-block Linear layers on the plane-fed GEMM (k_gemm.h): pre-split operand planes from LayerNorm / GroupNorm / attention / GEGLU, LDS-DMA only (the W3 weight copies are built when a model is built)"},
  {"gemm_p3_tile", 0, 0, "row tile of the plane-fed GEMM: 0 by shape, 256 / 128 / 64 forced"},
  {"gemm_p3_attn", 1, 1, "d=64 attention cores write the operand planes of to_out themselves (0: fp32 result + one conversion pass)"},
  {"gemm_p3_persist", 1, 1, "plane-fed GEMM: persistent blocks that prefetch the next tile's first chunk underneath the epilogue (0: one block per tile, n > 1: a grid of n blocks - tests)"},
  {"gemm_p3_ablate", 0, 0, "bench only: 1 no MFMAs, 2 no DMAs behind the prologue, 4 no epilogue (sdm_bench_gemm_p3)"},
  {"conv_up_phase", 1, 1, "up-sampling 3x3 convs (Upsample2D) as four 2x2-tap phase convs on the plane-fed GEMM (k_gemm.h, UP): 0 off (the 3x3 kernels on the up-sampled image), 1 the launches with at least two 256-row tiles per CU (up_phase_wins: measured), 2 every eligible launch (tests).  0 / non-0 is read when a model is built: the phase matrices are a derived weight layout"},
  {"conv_epi", 4, 4, "F8 kernels' epilogue: 4 register-direct stores + residual as accumulator init, 3 residual init only, 0 LDS-staged"},
  {"conv_xtile", 1, 1, "F8 3x3: cross-tile prefetch by the producer waves"},
  {"conv_f8_tpb", 0, 0, "F8: tiles per block (0 = by queue depth)"},
  {"conv_dma", 1, 1, "3x3 stride-1 256x128 tile: weights by LDS-DMA"},
  {"conv_dma_all", 0, 0, "keep a stage-ordered weight copy for every wide 3x3 layer, not only the split-precision ones (read when a model is built)"},
  {"conv_pc", -1, -1, "producer / consumer form of the split-precision DMA kernel: -1 by channel count, 0 off, 1 on"},
  {"conv_pc_min_cin", 256, 256, "conv_pc = -1: smallest Cin that takes the producer / consumer form"},
  {"conv_db", 0, 0, "512x128 double-buffered tile where the queue is deep"},
  {"trimap_skip", 1, 1, "VAE encoder, trimap images: output tiles inside a constant region of the trimap are not multiplied (k_misc.h cmask_*; exact). 0 = every tile"},
  {"conv_band_rows", 0, 0, "tile rows per XCD band of the convs that leave constant tiles out (0 = by image height)"},
  {"trimap_skip_min_rows", 512, 512, "smallest output height at which constant tiles are left out (measured at 1024^2: the 1024- and 512-row levels gain 3.7 + 1.6 ms, the 256-row level loses 0.7: too few of its 32 x 128-pixel tiles lie inside one region)"},
  {"conv_splitk", -1, -1, "split-K of the register-staged conv / GEMM kernels: -1 by shape (few tiles, long K), 0 off, n >= 2 forced where the shape allows"},
  {"force_cfg0", 0, 0, "always the 256x128 tile for 3x3 stride 1 (tests: fused GroupNorm at tiny sizes)"},
  {"no_gn_fuse", 0, 0, "never fuse the GroupNorm apply into the consuming conv"},
  {"split_lds_pad", 0, 0, "extra dynamic LDS of the register-staged split kernels (forces one block per CU)"},
  {"attn_f8", 1, 1, "Q.K^T residual terms of the d=64 split-precision attention on fp8 MFMAs"},
  {"attn_dense", 0, 0, "walk every key tile of the trimap-biased self-attention"},
  {"attn_pv_split", 0, 0, "residual terms of P.V too (fully split attention; tests)"},
  {"attn_nw", 0, 0, "waves per d=64 attention block: 0 by launch size, 4, 8"},
  {"attn_pipe", 1, 1, "8-wave split-precision d=64 attention: two-tile software pipeline"},
  {"attn_pipe4", 1, 1, "the same pipeline for the 4-wave launches (two K / three V^T buffers)"},
  {"attn_pp", 1, 1, "split-precision d=64 attention with fp32 output as a ping-pong of the block's wave halves (attn_d64_pp_kernel, 256 query rows per block): 0 off, 1 on, 2 on without the static priority of the younger half, 3 on with per-segment priority flips"},
  {"attn_pp_min_blocks", 128, 128, "attn_pp: launches with fewer 256-row blocks than this keep the 4-wave pipelines (0 in tests: the ping-pong kernel at any size)"},
  {"attn_ksplit", 0, 0, "key split of the d=64 split-precision attention: 0 by launch size (blocks that do not fill the chip's block slots a whole number of times), 1 off, 2 / 4 forced, 3 forced on the ping-pong kernel (ignored elsewhere: those launches run unsplit)"},
  {"attn512_pp", 0, 0, "d=512 attention (VAE mid-block): the ping-pong kernel (the block's two wave halves one phase apart, attn_d512_pp_kernel; bit-identical): 1 with s_setprio 1 for waves 4-7, 2 without (A/B), 0 = attn_d512_kernel.  Off: measured at 4 x 1024^2 it gains 0.08 ms per step, inside the run-to-run spread (profiles/r09_patch_tokens_ab.txt)"},
  {"cross_narrow", 1, 1, "cross_shared: the narrow form of the d = 64 cores on the shared operand (36 live columns: no Q.K^T step over columns 48..63, the softmax denominator from a row of ones in V^T instead of its own MFMAs; bit-identical).  0 = the full d = 64 program on an operand without the ones rows.  Read per forward"},
  {"cross_shared", 1, 1, "cross-attention on ONE key / value operand per forward, the patch matrix of the trimap latent (cross_patch_planes_kernel), with the K|V fold moved into q_shared / out_shared: 0 = every block's own kv_folded conv + transpose.  Read per forward"},
  {"attn_patch_tokens", 1, 1, "token order inside the U-Net transformers of a level whose latent is whole 8x8 patches and at least 64 wide (sdm_patch_tokens_ok): 64 consecutive tokens = an 8x8 patch, so the key tiles the trimap bias skips follow the foreground's shape (GroupNorm-apply in front of proj_in, the proj_out epilogue and the level's key bias carry the map).  0 = row-major pixel order everywhere.  Read per forward"},
  {"dbg_stats_poison", 0, 0, "tests: every partial-row statistics buffer is filled with 0xFF bytes (NaN) in front of the launch that writes it - a row the launch forgets shows in whatever reads it (the buffers are never cleared otherwise)"},
  {"precise_mask", -1, -1, "stages in split precision (-1 = the config's own mask; per-stage attribution experiments; read at sdm_create)"},
#ifdef SDM_EMU
  {"emu_arena_extra", 0, 0, "emulator build only, self-test of the arena check: the launch pass of a stand-alone op allocates one block its sizing pass did not"},
#endif
};
static OptEntry* opt_find(const char* name) {
  for (auto& o : g_opts) if (name && strcmp(o.name, name) == 0) return &o;
  return nullptr;
}
static int opt(const char* name) { OptEntry* o = opt_find(name); return o ? o->value : 0; }
// One process may run one engine per host thread (parallel.py MultiGpuEngine, ctypes releases the GIL).  Options are process-wide: a forward
// holds g_opt_mu shared from before its dry pass to the end of its launch pass, sdm_set_option / sdm_reset_options take it exclusively - an option
// can therefore never change between the pass that sizes the arena and the pass that launches (it waits for the forwards in flight).  The launch
// counters are a mutex-guarded map: a few hundred increments per step.
static std::shared_mutex g_opt_mu;
struct OptReadLock { std::shared_lock<std::shared_mutex> l; OptReadLock() : l(g_opt_mu) {} };
static std::mutex g_count_mu;
static std::map<std::string, long> g_kernel_counts;
static void count_kernel(const char* name) { std::lock_guard<std::mutex> g(g_count_mu); g_kernel_counts[name] += 1; }

// ------------------------------------------------------------------------------------------------
// conv tile configurations
// ------------------------------------------------------------------------------------------------
template <int NTAPS, int STRIDE, int TH, int TW, int BN, int KC, int WM, int WN, int DB = 0, int GNOK = 0>
static void launch_conv_t(const ConvParams& p_in, void* stream) {
  using C = ConvCfg<NTAPS, STRIDE, TH, TW, BN, KC, WM, WN, DB>;
  ConvParams p = p_in;
  p.tiles_m = (NTAPS == 9) ? sdm_cdiv(p.Wout, TW) * sdm_cdiv(p.Hout, TH)
                           : (int)(((p.rows_per_img ? (long)p.rows_per_img : p.M) + C::BM - 1) / C::BM);
  p.tiles_n = sdm_cdiv(p.Cout_pad, BN);
  const long total_m = (long)p.tiles_m * ((NTAPS == 9 || p.rows_per_img) ? p.N : 1);
  p.xcd_chunk = (int)((total_m + 7) / 8);
  const dim3 grid((unsigned)(8L * p.xcd_chunk * p.tiles_n), (unsigned)(p.ksplit > 1 ? p.ksplit : 1), 1);      // x: XCD-aware 1-D mapping in the kernel; y: split-K
  const size_t gn_extra = (size_t)(p.C0 + p.C1) * 8;                    // fused GroupNorm apply: the scale|shift table of the image follows the tiles in LDS
  if constexpr (!DB) {
    if (p.w_lo) {                  // precise mode: split-fp16 operands (fp32 activations only)
      using CS = ConvCfg<NTAPS, STRIDE, TH, TW, BN, KC, WM, WN, 0, 1>;
      const size_t lds_pad = (size_t)opt("split_lds_pad");   // experiment option: extra dynamic LDS (forces 1 block per CU)
      if (GNOK && p.gn_scale) {
        auto k = conv_mfma_kernel<NTAPS, STRIDE, TH, TW, BN, KC, WM, WN, 1, 0, GNOK, 1>;
        SDM_SET_SMEM(k, 160 * 1024);
        SDM_LAUNCH(k, grid, dim3(CS::NTHREADS), (size_t)CS::SMEM + gn_extra + lds_pad, stream, p);
      } else {
        auto k = conv_mfma_kernel<NTAPS, STRIDE, TH, TW, BN, KC, WM, WN, 1, 0, 0, 1>;
        SDM_SET_SMEM(k, 160 * 1024);
        SDM_LAUNCH(k, grid, dim3(CS::NTHREADS), CS::SMEM + lds_pad, stream, p);
      }
      return;
    }
  }
  if (GNOK && p.gn_scale) {
    const size_t smem = (size_t)C::SMEM + gn_extra;
    if (p.in_f32) {
      auto k = conv_mfma_kernel<NTAPS, STRIDE, TH, TW, BN, KC, WM, WN, 1, DB, GNOK>;
      SDM_SET_SMEM(k, C::SMEM + 1024 * 8);
      SDM_LAUNCH(k, grid, dim3(C::NTHREADS), smem, stream, p);
    } else {
      auto k = conv_mfma_kernel<NTAPS, STRIDE, TH, TW, BN, KC, WM, WN, 0, DB, GNOK>;
      SDM_SET_SMEM(k, C::SMEM + 1024 * 8);
      SDM_LAUNCH(k, grid, dim3(C::NTHREADS), smem, stream, p);
    }
    return;
  }
  if (p.in_f32) {
    auto k = conv_mfma_kernel<NTAPS, STRIDE, TH, TW, BN, KC, WM, WN, 1, DB, 0>;
    SDM_SET_SMEM(k, C::SMEM);
    SDM_LAUNCH(k, grid, dim3(C::NTHREADS), C::SMEM, stream, p);
  } else {
    auto k = conv_mfma_kernel<NTAPS, STRIDE, TH, TW, BN, KC, WM, WN, 0, DB, 0>;
    SDM_SET_SMEM(k, C::SMEM);
    SDM_LAUNCH(k, grid, dim3(C::NTHREADS), C::SMEM, stream, p);
  }
}

struct ConvCfgInfo { int TH, TW, BN, KC, WM; };
static const ConvCfgInfo kCfg3s1[] = {{8, 32, 128, 16, 2}, {4, 32, 64, 32, 4}, {8, 8, 64, 16, 2}, {16, 32, 128, 16, 4}, {8, 32, 32, 16, 4}, {8, 32, 64, 16, 2}};
static const ConvCfgInfo kCfg3s2[] = {{4, 32, 64, 16, 4}, {8, 8, 64, 16, 2}, {4, 32, 128, 16, 2}, {8, 32, 128, 16, 4}};
static const ConvCfgInfo kCfg1[] = {{8, 32, 128, 64, 2}, {4, 32, 64, 64, 4}, {8, 8, 64, 64, 2}, {8, 8, 64, 16, 2}, {8, 32, 128, 32, 2}};

static int conv_num_cfgs(int ntaps, int stride) { return ntaps == 9 ? (stride == 1 ? 6 : 4) : 5; }
static const ConvCfgInfo* conv_cfg_table(int ntaps, int stride) { return ntaps == 9 ? (stride == 1 ? kCfg3s1 : kCfg3s2) : kCfg1; }

static bool conv_cfg_ok(const ConvCfgInfo& c, const ConvParams& p) {
  const int Cin = p.C0 + p.C1;
  if (Cin % c.KC) return false;
  if (p.C1 > 0 && (p.C0 % c.KC)) return false;
  return true;
}

static int conv_pick_cfg(int ntaps, int stride, const ConvParams& p) {
  const ConvCfgInfo* t = conv_cfg_table(ntaps, stride);
  const int n = conv_num_cfgs(ntaps, stride);
  long best_blocks = -1;
  int best = -1;
  if (ntaps == 9 && stride == 1 && opt("force_cfg0") && conv_cfg_ok(t[0], p)) return 0;   // test option: exercise the 256x128 tile (+ fused GroupNorm) at tiny sizes
  const bool use_db = opt("conv_db") != 0;   // A/B option for the 512x128 double-buffered tile
  for (int i = 0; i < n; ++i) {
    if (!conv_cfg_ok(t[i], p)) continue;
    if (ntaps == 9 && stride == 1 && i >= 3) continue;          // cfg 3 / 4: variants of cfg 0, substituted below
    if (ntaps == 9 && stride == 2 && i >= 2) continue;          // cfg 2: forced only; cfg 3: substituted below
    if (ntaps == 1 && i >= 4) continue;                         // cfg 4: the fp32-input form of cfg 0, substituted below
    long blocks;
    if (ntaps == 9) {
      if (t[i].TW > 8 && p.Wout < 24) continue;   // 32-wide strips would be mostly padding
      blocks = (long)p.N * sdm_cdiv(p.Hout, t[i].TH) * sdm_cdiv(p.Wout, t[i].TW) * sdm_cdiv(p.Cout_pad, t[i].BN);
    } else {
      blocks = ((p.M + t[i].TH * t[i].TW - 1) / (t[i].TH * t[i].TW)) * sdm_cdiv(p.Cout_pad, t[i].BN);
    }
    if (best < 0) { best = i; best_blocks = blocks; }
    // first (largest) tile that still spreads over the chip.  Measured: a 3x3 stride-1 layer with 160 blocks of the 256x128 tile
    // beats 640 blocks of the 128x64 tile by 6-12 % (and 160 x 128x64 beats 320 x 64x64 by 22 %), so half a block per CU is
    // enough there; GEMMs and stride-2 layers keep the one-block-per-CU rule.
    const long enough = (ntaps == 9 && stride == 1) ? 128 : 256;
    if (blocks >= enough) {
      // cfg 3 (512-pixel tile, 1 block per CU) needs at least ~2 blocks per CU of its own to pay off
      if (use_db && ntaps == 9 && stride == 1 && i == 0 && (long)p.N * sdm_cdiv(p.Hout, 16) * sdm_cdiv(p.Wout, 32) * sdm_cdiv(p.Cout_pad, 128) >= 512) return 3;
      // thin outputs (conv_out layers, Cout <= 32): the same 256-pixel tile with 32 output channels instead of 128 (HBM-bound
      // layers: 128 -> 3 @1024^2 1.33 -> 0.63 ms)
      if (ntaps == 9 && stride == 1 && i == 0 && p.Cout_pad <= 32 && conv_cfg_ok(t[4], p)) return 4;
      // fewer than two rounds of the 256x128 tile (2 blocks per CU): the 256x64 tile (3 blocks per CU, twice the blocks) fills the
      // chip better - measured +5..17 % on the U-Net layers (320 ch @128^2, 640 @64^2, 1280 @32^2), -3..10 % on the large VAE layers
      // (not for layers with the fp8-residual weights: their 8-wave one-block-per-CU kernel on the 256x128 tile measured
      // 1.35-1.5x the 256x64 tile on exactly these shapes)
      if (ntaps == 9 && stride == 1 && i == 0 && blocks < 1024 && p.Cout_pad > 64 && !p.f8_hint && conv_cfg_ok(t[5], p)) return 5;
      // stride 2: 256 pixels x 128 channels on 8 waves halves the input re-reads per output channel (+25 % on the VAE
      // down-samplers) once there is a block for every CU
      if (ntaps == 9 && stride == 2 && i == 0 && conv_cfg_ok(t[3], p) &&
          (long)p.N * sdm_cdiv(p.Hout, 8) * sdm_cdiv(p.Wout, 32) * sdm_cdiv(p.Cout_pad, 128) >= 256) return 3;
      // fp32 activations into the 256x128 GEMM tile: K-chunks of 32 (the 64-channel chunk needs 64 staging registers on top of
      // the 128 accumulators and spills)
      if (ntaps == 1 && i == 0 && p.in_f32 && conv_cfg_ok(t[4], p)) return 4;
      return i;
    }
    if (blocks > best_blocks) { best = i; best_blocks = blocks; }
  }
  return best;
}

// Split-K for the register-staged kernels (k_conv.h, ConvParams::ksplit).  The 16x16 / 32x32 levels of the U-Net have a handful of
// 64- or 128-pixel tiles and K = 9 x 1280 ... 2560: one block walks up to 160 chunks with a global-load round trip in each, and at
// one image per call there are fewer blocks than CUs.  Splitting K puts s times the waves in flight; the partial sums (fp32, a few MB)
// are added by splitk_reduce_kernel, which also applies bias / residual / statistics.  Returns 1 when the layer is not split.
static int conv_pick_ksplit(int ntaps, int stride, int cfg, const ConvParams& p) {
  const int o = opt("conv_splitk");
  if (o == 0 || o == 1) return 1;
  const ConvCfgInfo& c = conv_cfg_table(ntaps, stride)[cfg];
  const int Cin = p.C0 + p.C1;
  auto valid = [&](int s) { return s >= 2 && Cin % (s * c.KC) == 0; };
  if (o >= 2) return valid(o) ? o : 1;
  const long blocks = (ntaps == 9) ? (long)p.N * sdm_cdiv(p.Hout, c.TH) * sdm_cdiv(p.Wout, c.TW) * sdm_cdiv(p.Cout_pad, c.BN)
                                   : ((p.M + c.TH * c.TW - 1) / (c.TH * c.TW)) * sdm_cdiv(p.Cout_pad, c.BN);
  // measured (tools/conv_splitk_ab.py, profiles/r04_conv_splitk_ab.txt), 1 and 4 images per call: layers with <= 320 blocks gain x1.1-3.0 from as
  // many splits as keep blocks x splits <= 1280 (3x3 at 16x16: 219 -> 85 us at one image, 253 -> 135 us at four; Linear 5120 -> 1280 at 32x32:
  // 156 -> 77 us); at 640 blocks and above splitting loses or is neutral
  const long kdepth = (long)Cin * ntaps;
  const long min_total = ntaps == 9 ? 2560 : 1280, min_part = ntaps == 9 ? 1152 : 320;
  if (blocks > 320 || kdepth < min_total) return 1;
  int best = 1;
  for (int s = 2; s <= 8; s *= 2)
    if (valid(s) && blocks * s <= 1280 && kdepth / s >= min_part) best = s;
  return best;
}

// F8 conv kernel: tiles a block runs back to back (the producer waves stage tile k+1 under the epilogue of tile k).  Only when
// every CU still gets a block: 160 tiles as 80 two-tile blocks measured 0.43 vs 0.26 ms.  The option conv_f8_tpb overrides (A/B).
// compute units of the current device (256 on an MI355X)
static int device_cus() {
#ifdef SDM_EMU
  return 256;
#else
  static std::atomic<int> cus{0};
  int c = cus.load(std::memory_order_relaxed);
  if (!c) {
    int dev = 0;
    hipDeviceProp_t pr;
    c = (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&pr, dev) == hipSuccess && pr.multiProcessorCount > 0) ? pr.multiProcessorCount : 256;
    cus.store(c, std::memory_order_relaxed);
  }
  return c;
#endif
}

static int conv_f8_tiles_per_block(long tiles) {
#ifdef SDM_EMU
  return tiles >= 6 ? 3 : (tiles >= 2 ? 2 : 1);
#else
  if (opt("conv_f8_tpb") >= 1 && opt("conv_f8_tpb") <= 8) return opt("conv_f8_tpb");
  const int cus = device_cus();
  // measured (profiles/r02_conv_f8_tiles_per_block.txt): 128->128 @1024^2 (64 tiles per CU) 490 / 504 / 516 TFLOP/s at 1 / 2 / 4 tiles per
  // block; 320->320 @128^2 (3 per CU) 542 / 455; 1280->1280 @32^2 (0.6 per CU) 575 / 299: only deep queues gain
  const long per_cu = tiles / cus;
  return per_cu >= 32 ? 4 : (per_cu >= 8 ? 2 : 1);
#endif
}

// Persistent grid of the F8 kernels (3x3 and 1x1): a block runs tpb of the vgrid tiles back to back.  Sets p.vgrid / p.tpb, returns the blocks to launch.
static unsigned f8_persistent_grid(ConvParams& p, unsigned vgrid) {
  p.vgrid = (int)vgrid;
  p.tpb = conv_f8_tiles_per_block((long)vgrid);
  const unsigned pg = (vgrid + p.tpb - 1) / p.tpb;
  return (pg + 7) & ~7u;              // block id % 8 = XCD: the stride between a block's tiles stays a multiple of 8
}

// 256 px x 128 co, 3x3 stride 1, weights through the LDS-DMA stage ring (k_conv.h, DMAB): fp16 / fp32 activations, optional fused
// GroupNorm, optional split precision
static void launch_conv_dma(const ConvParams& p_in, void* stream) {
  ConvParams p = p_in;
  p.tiles_m = sdm_cdiv(p.Wout, 32) * sdm_cdiv(p.Hout, 8);
  p.tiles_n = sdm_cdiv(p.Cout_pad, 128);
  const long total_m = (long)p.tiles_m * p.N;
  p.xcd_chunk = (int)((total_m + 7) / 8);
  if (p.tile_flag) {
    // some tiles of some images will be left out (ConvParams::tile_flag): bands of a few tile rows of EVERY image go round-robin over the XCDs, so
    // that no XCD owns only the images (or only the image regions) that are skipped
    const int npx = sdm_cdiv(p.Wout, 32), rows = sdm_cdiv(p.Hout, 8);
    const int br = opt("conv_band_rows") > 0 ? opt("conv_band_rows") : std::max(1, std::min(4, rows / 16));
    p.band = br * npx;
    p.img_chunk = sdm_cdiv(p.tiles_m, 8 * p.band) * p.band;
    p.xcd_chunk = p.N * p.img_chunk;
  }
  const dim3 grid((unsigned)(8L * p.xcd_chunk * p.tiles_n), 1, 1);
  const bool gn = p.gn_scale != nullptr, split = p.w_lo != nullptr;
  const size_t gn_extra = gn ? (size_t)(p.C0 + p.C1) * 8 : 0;
#define SDM_DMA_CASE(F32, GNF, SPL, PCF)                                                                     \
  do {                                                                                                       \
    using CD = ConvCfg<9, 1, 8, 32, 128, 16, 2, 2, 0, SPL, 1, PCF>;                                          \
    auto k = conv_mfma_kernel<9, 1, 8, 32, 128, 16, 2, 2, F32, 0, GNF, SPL, 1, PCF>;                         \
    SDM_SET_SMEM(k, 160 * 1024);                                                                             \
    SDM_LAUNCH(k, grid, dim3(CD::LAUNCH_THREADS), (size_t)CD::SMEM + gn_extra, stream, p);                   \
  } while (0)
  if (split && p.f8) {          // fp8-residual producer / consumer kernel (32-channel chunks; no GroupNorm table in LDS)
    using CD = ConvCfg<9, 1, 8, 32, 128, 32, 2, 2, 0, 1, 1, 1, 1>;
    const unsigned pg = f8_persistent_grid(p, grid.x);
#define SDM_F8_CASE(GNF)                                                                                     \
  do {                                                                                                       \
    auto k = conv_mfma_kernel<9, 1, 8, 32, 128, 32, 2, 2, 1, 0, GNF, 1, 1, 1, 1>;                            \
    SDM_SET_SMEM(k, 160 * 1024);                                                                             \
    SDM_LAUNCH(k, dim3(pg, 1, 1), dim3(CD::LAUNCH_THREADS), (size_t)CD::SMEM_F8, stream, p);                 /* LDS map: ConvCfg (k_conv.h) */ \
  } while (0)
    count_kernel(gn ? "conv3x3_f8<gn>" : "conv3x3_f8");
    if (gn) SDM_F8_CASE(1); else SDM_F8_CASE(0);
#undef SDM_F8_CASE
  }
  else if (split && p.pc) { count_kernel("conv3x3_pc"); if (gn) SDM_DMA_CASE(1, 1, 1, 1); else SDM_DMA_CASE(1, 0, 1, 1); }
  else if (split) { if (gn) SDM_DMA_CASE(1, 1, 1, 0); else SDM_DMA_CASE(1, 0, 1, 0); }
  else if (p.in_f32) { if (gn) SDM_DMA_CASE(1, 1, 0, 0); else SDM_DMA_CASE(1, 0, 0, 0); }
  else { if (gn) SDM_DMA_CASE(0, 1, 0, 0); else SDM_DMA_CASE(0, 0, 0, 0); }
#undef SDM_DMA_CASE
}

// Linear / 1x1 GEMM, 256 rows x 128 channels, fp8-residual producer / consumer kernel (k_conv.h, F8 with NTAPS = 1)
static void launch_gemm_f8(const ConvParams& p_in, void* stream) {
  using CD = ConvCfg<1, 1, 8, 32, 128, 32, 2, 2, 0, 1, 1, 1, 1>;
  ConvParams p = p_in;
  p.tiles_m = (int)(((p.rows_per_img ? (long)p.rows_per_img : p.M) + CD::BM - 1) / CD::BM);
  p.tiles_n = sdm_cdiv(p.Cout_pad, 128);
  const long total_m = (long)p.tiles_m * (p.rows_per_img ? p.N : 1);
  p.xcd_chunk = (int)((total_m + 7) / 8);
  const unsigned pg = f8_persistent_grid(p, (unsigned)(8L * p.xcd_chunk * p.tiles_n));
  count_kernel("gemm_f8");
  auto k = conv_mfma_kernel<1, 1, 8, 32, 128, 32, 2, 2, 1, 0, 0, 1, 1, 1, 1>;
  SDM_SET_SMEM(k, 160 * 1024);
  SDM_LAUNCH(k, dim3(pg, 1, 1), dim3(CD::LAUNCH_THREADS), (size_t)CD::SMEM_F8, stream, p);      // LDS map: ConvCfg (k_conv.h)
}

// ---- plane-fed GEMM (k_gemm.h): tile = (64 * MT) rows x 128 channels, 4 waves; NS LDS stages (2 stages of the 256-row tile: two blocks per CU) ----
template <int MT, int EPI, int UP = 0, int PT = 0>
static void launch_gemm_p3_t(GemmP3Params p, void* stream) {
  constexpr int BM = 64 * MT, NS = 2, SMEM = NS * (BM * 96 + 128 * 128);
  const long rows = p.rows_per_img ? (long)p.rows_per_img : p.M;
  p.tiles_per_img = (int)((rows + BM - 1) / BM);
  p.tiles_m = p.tiles_per_img * (p.rows_per_img ? (int)(p.M / p.rows_per_img) : 1);
  p.tiles_n = sdm_cdiv(p.N, 128) * (UP ? 4 : 1);      // (UP: the tile id's N part is phase * N tiles + N tile, k_gemm.h)
  unsigned grid;
  if (p.tiles_m >= 8) { p.xcd_chunk = (p.tiles_m + 7) / 8; grid = (unsigned)(8L * p.xcd_chunk * p.tiles_n); }
  else { p.xcd_chunk = 0; grid = (unsigned)(p.tiles_m * p.tiles_n); }
  // persistent grid: as many blocks as the chip holds at once (a multiple of 8: a block's tiles stay on its XCD's M range), each walks its tiles as one
  // DMA stream (k_gemm.h); the option gemm_p3_persist = 0 launches one block per tile
  if (const int pp = opt("gemm_p3_persist")) {
    const unsigned slots = pp > 1 ? (unsigned)pp : ((unsigned)(device_cus() * ((SMEM <= 80 * 1024) ? 2 : 1)) & ~7u);      // (pp > 1: forced grid, tests)
    if (slots >= 1 && grid > slots) grid = slots;
  }
  auto k = gemm_p3_kernel<MT, 2, EPI, NS, UP, PT>;
  SDM_SET_SMEM(k, SMEM);
#ifndef SDM_EMU
  if (opt("gemm_p3_ablate") & 256) {      // lab: resident blocks per CU as the runtime sees them
    int nb = -1;
    (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k, 256, (size_t)SMEM);
    fprintf(stderr, "[gemm_p3] tile %d stages %d epi %d: %d bytes of LDS, %d blocks per CU, grid %u\n", BM, NS, EPI, SMEM, nb, grid);
  }
#endif
  SDM_LAUNCH(k, dim3(grid, 1, 1), dim3(256), (size_t)SMEM, stream, p);
}
template <int EPI>
static void launch_gemm_p3_e(const GemmP3Params& p, int bm, void* stream) {
  if (bm == 256) launch_gemm_p3_t<4, EPI>(p, stream);
  else if (bm == 128) launch_gemm_p3_t<2, EPI>(p, stream);
  else launch_gemm_p3_t<1, EPI>(p, stream);
}
// row tile: the largest of 256 / 128 / 64 that still gives every CU a block (the option gemm_p3_tile forces one)
static int gemm_p3_pick_bm(long M, int N, int rows_per_img, int phases = 1) {
  const int forced = opt("gemm_p3_tile");
  if (forced == 256 || forced == 128 || forced == 64) return forced;
  const long tn = (long)sdm_cdiv(N, 128) * phases;
  const long imgs = rows_per_img ? M / rows_per_img : 1, rows = rows_per_img ? rows_per_img : M;
  const int cus = device_cus();
  for (int bm : {256, 128}) if (imgs * ((rows + bm - 1) / bm) * tn >= cus) return bm;
  return 64;
}
// proj_out of a transformer in patch token order (GemmP3Params::pt_W): its own instantiations of epilogues 0 / 4, so that every other launch keeps its code
template <int EPI>
static void launch_gemm_p3_tokens(const GemmP3Params& p, int bm, void* stream) {
  if (bm == 256) launch_gemm_p3_t<4, EPI, 0, 1>(p, stream);
  else if (bm == 128) launch_gemm_p3_t<2, EPI, 0, 1>(p, stream);
  else launch_gemm_p3_t<1, EPI, 0, 1>(p, stream);
}
static void launch_gemm_p3(const GemmP3Params& p, int epi, void* stream) {
  const int bm = gemm_p3_pick_bm(p.M, p.N, p.rows_per_img);
  if (p.pt_W) {
    count_kernel("gemm_p3_tokens");
    if (epi == 4) launch_gemm_p3_tokens<4>(p, bm, stream); else launch_gemm_p3_tokens<0>(p, bm, stream);
    return;
  }
  switch (epi) {
    case 0: launch_gemm_p3_e<0>(p, bm, stream); break;
    case 1: launch_gemm_p3_e<1>(p, bm, stream); break;
    case 2: launch_gemm_p3_e<2>(p, bm, stream); break;
    case 3: launch_gemm_p3_e<3>(p, bm, stream); break;
    default: launch_gemm_p3_e<4>(p, bm, stream); break;
  }
}

// up-sampling phase convs (k_gemm.h, UP): epilogue 0 (fp32) or 4 (+ statistics)
static void launch_gemm_p3_up(const GemmP3Params& p, int epi, int bm, void* stream) {
  if (epi == 4) {
    if (bm == 256) launch_gemm_p3_t<4, 4, 1>(p, stream); else if (bm == 128) launch_gemm_p3_t<2, 4, 1>(p, stream); else launch_gemm_p3_t<1, 4, 1>(p, stream);
  } else {
    if (bm == 256) launch_gemm_p3_t<4, 0, 1>(p, stream); else if (bm == 128) launch_gemm_p3_t<2, 0, 1>(p, stream); else launch_gemm_p3_t<1, 0, 1>(p, stream);
  }
}

static int launch_conv(int ntaps, int stride, int cfg, const ConvParams& p, void* stream) {
  if (ntaps == 9 && stride == 1) {
    switch (cfg) {
      case 0:
        if (p.w_dma) { launch_conv_dma(p, stream); return 0; }
        launch_conv_t<9, 1, 8, 32, 128, 16, 2, 2, 0, 1>(p, stream); return 0;   // 256 px x 128 co, fused-GroupNorm variant
      case 1: launch_conv_t<9, 1, 4, 32, 64, 32, 4, 1>(p, stream); return 0;
      case 2: launch_conv_t<9, 1, 8, 8, 64, 16, 2, 1>(p, stream); return 0;
      case 3: launch_conv_t<9, 1, 16, 32, 128, 16, 4, 2, 1>(p, stream); return 0;   // 512 px x 128 co, 8 waves, swizzled double-buffered LDS tiles
      case 4: launch_conv_t<9, 1, 8, 32, 32, 16, 4, 1, 0, 1>(p, stream); return 0;   // 256 px x 32 co: thin-output convs (conv_out), fused GroupNorm
      case 5: launch_conv_t<9, 1, 8, 32, 64, 16, 2, 2, 0, 1>(p, stream); return 0;   // 256 px x 64 co: 3 blocks per CU, for layers with few tiles; fused GroupNorm
    }
  } else if (ntaps == 9 && stride == 2) {
    switch (cfg) {
      case 0: launch_conv_t<9, 2, 4, 32, 64, 16, 4, 1>(p, stream); return 0;
      case 1: launch_conv_t<9, 2, 8, 8, 64, 16, 2, 1>(p, stream); return 0;
      case 2: launch_conv_t<9, 2, 4, 32, 128, 16, 2, 2>(p, stream); return 0;
      case 3: launch_conv_t<9, 2, 8, 32, 128, 16, 4, 2>(p, stream); return 0;
    }
  } else if (ntaps == 1) {
    switch (cfg) {
      case 0: launch_conv_t<1, 1, 8, 32, 128, 64, 2, 2>(p, stream); return 0;
      case 1: launch_conv_t<1, 1, 4, 32, 64, 64, 4, 1>(p, stream); return 0;
      case 2: launch_conv_t<1, 1, 8, 8, 64, 64, 2, 1>(p, stream); return 0;
      case 3: launch_conv_t<1, 1, 8, 8, 64, 16, 2, 1>(p, stream); return 0;
      case 4:
        if (p.f8 && p.w_dma) { launch_gemm_f8(p, stream); return 0; }
        launch_conv_t<1, 1, 8, 32, 128, 32, 2, 2>(p, stream); return 0;
    }
  }
  return -1;
}

// split-K launch: the conv kernel with grid.y = ksplit writes fp32 partial sums to the workspace, splitk_reduce_kernel finishes the layer
// (bias, output scale, residual, store format, statistics with one partial row per kSplitKRows rows of an image)
static const int kSplitKRows = 64;
static int launch_conv_splitk(int ntaps, int stride, int cfg, const ConvParams& p, int ksplit, float* ws, void* stream) {
  ConvParams ps = p;
  ps.out = ws; ps.out_f32 = 1; ps.Cout_store = p.Cout_pad; ps.out_ch_off = 0; ps.Cout_valid = p.Cout_pad;
  ps.bias = nullptr; ps.bias_sel = nullptr; ps.res = nullptr; ps.out_scale = 1.0f; ps.stats = nullptr; ps.rows_per_img = 0;
  ps.ksplit = ksplit; ps.ks_stride = (size_t)p.M * p.Cout_pad;
  const int rc = launch_conv(ntaps, stride, cfg, ps, stream);
  if (rc != 0) return rc;
  const int bpi = sdm_cdiv(p.Hout * p.Wout, kSplitKRows);
  SplitKReduceParams q;
  memset(&q, 0, sizeof(q));
  q.ws = ws; q.ksplit = ksplit; q.ks_stride = ps.ks_stride; q.ws_C = p.Cout_pad;
  q.rows_per_img = p.Hout * p.Wout; q.rb = kSplitKRows; q.blocks_per_img = bpi;
  q.bias = p.bias; q.bias_sel = p.bias_sel; q.Cout_pad = p.Cout_pad;
  q.res = p.res; q.res_f32 = p.res_f32; q.res_C = p.res_C; q.out_scale = p.out_scale;
  q.out = p.out; q.out_f32 = p.out_f32; q.Cout_store = p.Cout_store; q.out_ch_off = p.out_ch_off; q.Cout_valid = p.Cout_valid;
  q.stats = p.stats;
  SDM_LAUNCH(splitk_reduce_kernel, dim3((unsigned)(p.N * bpi), (unsigned)sdm_cdiv(p.Cout_valid, 64), 1), dim3(256), 0, stream, q);
  return 0;
}

// ------------------------------------------------------------------------------------------------
// engine data structures
// ------------------------------------------------------------------------------------------------
// Residual terms of the split-precision 3x3 convs on fp8 operands (k_conv.h, F8): default on; the option conv_f8 = 0 keeps them on fp16
// (the round-2 "fp16x3" arithmetic everywhere).  Read when a model is built: the weight copy is packed for one of the two.
static bool conv_f8_enabled() { return opt("conv_f8") != 0; }

static bool gemm_f8_enabled() { return opt("gemm_f8") != 0; }

// epilogue of the F8 kernels (ConvParams::epi_mode): 4 = register-direct 16-byte stores + residual as the accumulators' initial value
// (default), 3 = LDS-staged stores + residual as initial value, 0 = LDS-staged stores, residual added in the epilogue.  Read per launch:
// A/B hook.
static int conv_epi_mode() {
  const int v = opt("conv_epi");
  return (v == 0 || v == 3 || v == 4) ? v : 4;
}

// Residual terms of Q.K^T in the split-precision attention cores on fp8 MFMAs (k_attn.h, PREC = 3; q / k arrive as fp16 + e5m2 pair planes):
// default on; the option attn_f8 = 0 keeps them on fp16 MFMAs (PREC = 2, fp16 hi | lo planes).  Read per forward: A/B hook.
static bool attn_f8_enabled() { return opt("attn_f8") != 0; }

// F8 3x3 kernels: cross-tile prefetch by the producer waves (k_conv.h); the option conv_xtile = 0 disables.  Read per launch: A/B hook.
static bool conv_xtile_enabled() { return opt("conv_xtile") != 0; }

static int gemm_f8_min_k() { return opt("gemm_f8_min_k"); }

struct ConvL {
  std::string name;
  int ntaps = 1, I = 0, O = 0, Cin_pad = 0, Cout_pad = 0, geglu = 0;
  size_t w_off = 0, b_off = 0;
  half_t* w = nullptr;
  float* b = nullptr;
  // precise mode (sdm_config::precise_mask has the layer's stage bit): weights are packed as fp16 pairs w * 2^w_exp = hi + lo
  int stage = 0, split = 0, w_exp = 0;
  size_t wlo_off = 0;
  half_t* w_lo = nullptr;
  // 3x3 layers wide enough for the 256x128 tile also keep their weights in the stage order of the DMA-weight kernels
  size_t wdma_off = 0, wdma_bytes = 0;
  half_t* w_dma = nullptr;
  int f8 = 0;                 // w_dma holds the fp8-residual layout (F8 conv kernel) instead of the stage-ordered hi | lo pair
  int f8_exp = 8;             // f8: the layer's e4m3 weight scale 2^f8_exp, the largest power of two with max|w| * 2^f8_exp <= 448 (derive_layer)
  // Linear layers of the split-precision stages also keep the W3 layout of the plane-fed GEMM (k_gemm.h; same f8_exp)
  size_t w3_off = 0, w3_bytes = 0;
  unsigned char* w3 = nullptr;
  // 3x3 layers behind a nearest x2 up-sample (Upsample2D): the four phase matrices [4 * Cin_pad][Cout_pad] in the W3 layout (k_gemm.h, UP), with
  // their own e4m3 scale 2^up_exp from the largest SUMMED weight
  int up = 0;                 // the model runs the layer with ConvArgs::up = 1
  size_t wup_off = 0, wup_bytes = 0;
  unsigned char* wup = nullptr;
  int up_exp = 8;
  size_t w_bytes() const { return (size_t)Cin_pad * ntaps * Cout_pad * 2; }      // K16: each of w and w_lo
  size_t b_bytes() const { return (size_t)Cout_pad * 4; }
};
static const int kSplitWeightExp = 8;      // pre-scale 2^8: typical |w| ~ 1e-2 .. 1 -> low parts ~ 1e-3 .. 1e-1 * 2^-4: fp16-normal

static ConvL make_layer(const std::string& name, int ntaps, int I, int O, int geglu, int split) {
  ConvL L;
  L.name = name; L.ntaps = ntaps; L.I = I; L.O = O; L.geglu = geglu;
  L.Cin_pad = rup(I, 16);
  L.Cout_pad = rup(O, geglu ? 64 : 32);
  L.split = split ? 1 : 0;
  L.w_exp = split ? kSplitWeightExp : 0;
  return L;
}

// Which derived weight layouts a layer of a given shape can carry - the ONE statement of it, for the model's layers (Builder::conv) and for
// the temporary layers of the single-operator hooks (sdm_hooks.h TempLayer) alike.  The predicates hold what the kernels need; policy that only
// the model applies is passed in by its call site and is deliberately absent from the hooks, which build a layout for every eligible layer:
//   stage-ordered 3x3 copy   model: split-precision layers only, or all with conv_dma_all (measured +4..6 % there; neutral with fp16 operands,
//                            where the register-staged kernel stays);  hooks: every eligible layer - how the fp16 DMA kernel is op-tested
//   fp8-residual GEMM copy   model: K >= gemm_f8_min_k;  hooks: any K (small-K op tests of the 8-wave GEMM)
//   W3                       model: with conv_f8 and gemm_p3;  hooks: the conv hook never, the plane-fed GEMM hooks always
static bool layer_takes_dma3x3(const ConvL& L) { return L.ntaps == 9 && L.Cout_pad >= 128 && !L.geglu; }
// Linear / 1x1 layers of the split-precision stages: fp8-residual copy for the 8-wave GEMM kernel (k_conv.h, F8 with NTAPS = 1), used when the
// launch takes the 256 x 128 tile
static bool layer_takes_gemm_f8(const ConvL& L) {
  return L.ntaps == 1 && L.split && L.Cout_pad >= 128 && L.Cin_pad % 32 == 0 && conv_f8_enabled() && gemm_f8_enabled();
}
// Linear layers of a split-precision stage whose K splits into 32-channel chunks: W3 copy for the plane-fed GEMM (k_gemm.h)
static bool layer_takes_w3(const ConvL& L) { return L.ntaps == 1 && L.split && L.Cin_pad % 32 == 0 && L.Cin_pad >= 32; }
// 3x3 layers of a split-precision stage whose channels split into 32-channel chunks: phase matrices for the up-sampling path (k_gemm.h, UP)
//   model: the Upsample2D layers, NEXT TO their stage-ordered copy - which of the two a launch takes depends on its size (up_phase_wins), and the
//   same layer sees every size;  hooks: every eligible layer run with up = 1
static bool layer_takes_up_phase(const ConvL& L) {
  return L.ntaps == 9 && L.split && !L.geglu && L.Cin_pad % 32 == 0 && L.Cin_pad >= 32 && conv_f8_enabled() && opt("conv_up_phase") != 0;
}
// Which up-sampling launches take the phase path.  Measured per launch at 4 x 1024^2 (profiles/NOTES.md, "Up-sampling convs as phase convs"): launch +
// plane pre-pass beat the F8 3x3 launch by 1.33 - 1.66x on the five layers with 800 ... 66 000 tiles of 256 rows x 128 channels and lose 13 % on the one
// with 320 (1280 -> 1280 at 16^2 -> 32^2: 0.63 of one round of the chip's 512 resident blocks, half of its row tiles a quarter full; the 128- and
// 64-row tiles measured slower still).  The line is drawn at one full round.
static bool up_phase_wins(int N, int H, int W, int Cout_pad) {
  if (opt("conv_up_phase") >= 2) return true;
  const long tiles = (long)N * sdm_cdiv((H + 2) * (W + 2), 256) * 4 * sdm_cdiv(Cout_pad, 128);
  return tiles >= 2L * device_cus();
}
// sizes of the derived copies the caller wants and the layer can carry (0: none), and which of the two layouts w_dma holds
static void layer_choose_layouts(ConvL& L, bool want_dma3x3, bool want_gemm_f8, bool want_w3, bool want_up_phase = false) {
  if (want_up_phase && layer_takes_up_phase(L)) L.wup_bytes = (size_t)16 * L.Cin_pad * L.Cout_pad * 4;
  if (want_dma3x3 && layer_takes_dma3x3(L)) {
    L.wdma_bytes = L.w_bytes() * (L.split ? 2 : 1);
    L.f8 = (L.split && L.Cin_pad % 32 == 0 && conv_f8_enabled()) ? 1 : 0;      // same bytes, fp8-residual layout
  }
  if (want_gemm_f8 && layer_takes_gemm_f8(L)) { L.wdma_bytes = L.w_bytes() * 2; L.f8 = 1; }
  if (want_w3 && layer_takes_w3(L)) L.w3_bytes = L.w_bytes() * 2;
}
struct NormL {
  int C = 0;
  size_t g_off = 0, b_off = 0;
  float* g = nullptr;
  float* b = nullptr;
};
enum SlotKind { SLOT_CONV_W, SLOT_CONV_B, SLOT_NORM_G, SLOT_NORM_B, SLOT_HOST };
struct Slot {
  int kind = 0, layer = -1, co_off = 0, ci_off = 0;
  float w_scale = 1.0f;    // SLOT_CONV_W: constant folded into the weight before the fp16 rounding (attention logit scale in to_q)
  std::vector<int64_t> shape;
  size_t host_off = 0;     // SLOT_HOST: float offset in the host blob
  bool host_too = false;   // a packed slot whose fp32 tensor is ALSO kept in the host blob at host_off (a finalize-time fold reads it)
  bool loaded = false;
};
struct ResB { int norm1 = -1, conv1 = -1, norm2 = -1, conv2 = -1, sc = -1, temb = -1, cin = 0, cout = 0; };
struct VaeAttnB { int gn = -1, qkv = -1, out = -1, C = 0; };
struct TfB { int gn, proj_in, ln1, qkv1, o1, ln2, q2, kv2, o2, ln3, ff1, ff2, proj_out, C, heads; size_t k_hoff, v_hoff;
             int q2s, o2s; size_t q_hoff, o_hoff, ob_hoff; };      // shared-operand form of the cross-attention (fold_cross_shared)
struct TembL { size_t w_hoff = 0, b_hoff = 0, cb_hoff = 0; int cout = 0, cout_pad = 0; float* table = nullptr; };

struct T {  // NHWC activation tensor living in the arena
  size_t off = 0, bytes = 0;
  void* p = nullptr;
  int N = 0, H = 0, W = 0, C = 0, f32 = 0;
  bool want_stats = false;      // the producing conv should emit fused GroupNorm statistics
  float* stats = nullptr;       // [N][srows][C][2] partial {sum, sumsq} rows written by the producing conv epilogue
  int srows = 0;
  size_t soff = 0, sbytes = 0;
  unsigned char* cmask = nullptr;   // optional class plane [N][H][W] of a piecewise-constant batch (k_misc.h cmask_*): set by vae_encode on the encoder input,
  size_t cm_off = 0, cm_bytes = 0;  // propagated by op_conv through 3x3 convs; owned by the tensor (freed with it)
  int cm_n0 = 0;                    // first image of the batch that carries classes (the rgb images in front of it have none)
  long rows() const { return (long)N * H * W; }
};

// activation element formats (T::f32): 0 fp16, 1 fp32, 2 two fp16 planes hi | lo (split-precision attention operands),
// 3 fp16 plane hi + e5m2 pair plane (the same, with the residual operands of Q.K^T already in fp8: ConvParams::out_f32),
// 4 "P3": fp16 plane hi + one plane of e5m2 residual bytes, 3 bytes per element - the operand format of the plane-fed GEMM (k_gemm.h)
static const int kFmtP3 = 4;
static inline size_t fmt_bytes(int f) { return f == kFmtP3 ? 3 : (f ? 4 : 2); }
static const int kMinVariantRows = 8;     // initial rows of the per-ResBlock bias tables (one row per distinct conditioning); grows on demand
// conditioning of one image: opacity class + either 4 box coordinates (kind 0: bbox_embedding) or N point coordinates
// (kind 1: point_embedding), meta_arch.py:147-197 / replace.py:446-457
struct Variant {
  int trans = 0, kind = 0;
  std::vector<float> c;
  bool operator==(const Variant& o) const { return trans == o.trans && kind == o.kind && c == o.c; }
};

struct ProfRec { std::string name, desc; double flops, bytes;
#ifndef SDM_EMU
  hipEvent_t e0, e1;
#endif
};

struct sdm_ctx {
  sdm_config cfg;
  int device = 0;
  const unsigned char* dbg_cmask = nullptr;      // test hook (sdm_debug_set_input_cmask): class plane of the next sdm_op_conv_ex input
  void* stream = nullptr;
  bool own_stream = false;
  std::string err;
  // weights
  std::vector<ConvL> convs;
  std::vector<NormL> norms;
  std::unordered_map<std::string, Slot> slots;
  std::vector<std::string> slot_order;
  unsigned char* warena = nullptr;
  size_t warena_bytes = 0, canon_bytes = 0;      // whole arena; its leading canonical part (the exported / imported blob)
  std::vector<float> hostblob;
  int64_t n_loaded = 0, n_ignored = 0;
  std::vector<std::string> missing;
  bool finalized = false;
  void* stage = nullptr;
  size_t stage_bytes = 0;
  // asynchronous weight pipeline: a ring of (pinned host, device) staging pairs; tensor i+1 is converted
  // into pinned memory on the CPU while tensor i is copied and packed on the GPU - no host synchronisation per tensor
  struct LoadSlot {
    void* host = nullptr; void* dev = nullptr; size_t cap = 0; bool busy = false;
#ifndef SDM_EMU
    hipEvent_t done = nullptr;
#endif
  };
  static const int kLoadSlots = 3;
  LoadSlot load_ring[kLoadSlots];
  int load_next = 0;
  // model structure
  int enc_conv_in, enc_norm_out, enc_conv_out, quant, post_quant, dec_conv_in, dec_norm_out, dec_conv_out;
  std::vector<std::vector<ResB>> enc_res, dec_res;
  std::vector<int> enc_down, dec_up;
  ResB enc_mid0, enc_mid1, dec_mid0, dec_mid1;
  VaeAttnB enc_attn, dec_attn;
  int u_conv_in, u_aux, u_norm_out, u_conv_out;
  std::vector<std::vector<ResB>> u_down_res, u_up_res;
  std::vector<std::vector<TfB>> u_down_tf, u_up_tf;
  std::vector<int> u_down_ds, u_up_us;
  ResB u_mid0, u_mid1;
  TfB u_midtf;
  std::vector<TembL> tembs;
  size_t h_time1w, h_time1b, h_time2w, h_time2b, h_bbox1w, h_bbox1b, h_bbox2w, h_bbox2b, h_auxw, h_auxb;
  size_t h_point1w, h_point1b, h_point2w, h_point2b;
  std::vector<Variant> variants;
  int variant_cap = 0;         // rows allocated in every TembL::table
  int act_f32 = 0;             // precise_mask != 0: every activation that is fp16 in the fast graph is kept in fp32
  int* d_bias_sel = nullptr;   // [max batch]
  int bias_sel_cap = 0;
  // activation arena
  unsigned char* arena = nullptr;
  size_t arena_bytes = 0;
  bool dry = false;
  size_t peak = 0;
  std::map<size_t, size_t> freelist;  // off -> size
  size_t arena_top = 0;
  // dry / launch pass agreement (arena_pass_begin / arena_pass_end): the sizing pass records the size of every talloc in order, the launch pass
  // compares each of its own with it.  From the first that differs - or would end past arena_bytes - on, allocations get a buffer of their own
  // outside the arena (`aside`, released at the end of the pass) and the pass fails with SDM_ERR_ARENA naming that first one.
  std::vector<size_t> atrace;
  size_t atrace_i = 0;
  bool adiverged = false;
  std::string adiv_msg;
  std::vector<void*> aside;
  // io staging
  void* io_in = nullptr; size_t io_in_bytes = 0;
  void* io_out = nullptr; size_t io_out_bytes = 0;
  // timing / profiling
  float last_ms = 0.f;
  bool prof_on = false;
  std::vector<ProfRec> prof;
  struct ProfAgg { std::string name; float ms; int64_t n; double flops, bytes; };
  std::vector<ProfAgg> prof_agg;
  std::string prof_dump;   // per-launch CSV of the last profiled forward
#ifndef SDM_EMU
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  hipEvent_t ev_in = nullptr, ev_out = nullptr;   // ordering against the caller's stream (SDM_PTR_DEVICE calls)
#endif
};

static std::string g_create_err;

#define SDM_FAIL(ctx, code, ...)                       \
  do {                                                 \
    char buf_[512];                                    \
    snprintf(buf_, sizeof(buf_), __VA_ARGS__);         \
    (ctx)->err = buf_;                                 \
    return (code);                                     \
  } while (0)

#define SDM_CHECK_DEV(ctx, expr)                                                              \
  do {                                                                                        \
    int e_ = (expr);                                                                          \
    if (e_ != 0) SDM_FAIL(ctx, SDM_ERR_HIP, "%s failed: %s (%s:%d)", #expr, dev_errstr(e_), __FILE__, __LINE__); \
  } while (0)

#define TRY(x) do { int rc_ = (x); if (rc_) return rc_; } while (0)

// ------------------------------------------------------------------------------------------------
// model construction (mirrors comfyui-sdmatte_amd/weights.py::weight_schema)
// ------------------------------------------------------------------------------------------------
struct Builder {
  sdm_ctx* e;
  size_t woff = 0;         // canonical region: K16 weights (hi | lo), biases, norm affine - what sdm_export_weight_blob carries
  size_t doff = 0;         // derived region (behind the canonical one): DMA-ordered / fp8-residual copies, rebuilt by sdm_finalize_weights
  int stage = 0;           // sdm_precise_stage of the layers being built
  explicit Builder(sdm_ctx* c) : e(c) {}
  int conv(const std::string& name, int ntaps, int I_pad16_src, int O, int geglu = 0, int up = 0) {
    ConvL L = make_layer(name, ntaps, I_pad16_src, O, geglu, e->cfg.precise_mask & stage);
    L.stage = stage; L.up = up;
    L.w_off = woff; woff += rupz(L.w_bytes(), 256);
    L.b_off = woff; woff += rupz(L.b_bytes(), 256);
    if (L.split) { L.wlo_off = woff; woff += rupz(L.w_bytes(), 256); }
    // The model's own policy on top of what a layer can carry (layer_choose_layouts).  The fp8-residual GEMM copy has a threshold on K: a GEMM
    // has no operand reuse across taps, so the producer waves (one 32 KB activation tile converted per 1024 MFMA cycles) set the pace: measured
    // against the 4-wave kernel x1.2-1.5 for K = 1280 ... 5120, x0.84-1.0 for K <= 640 (profiles/r02_gemm_f8_ab.txt)
    layer_choose_layouts(L, L.split || opt("conv_dma_all") != 0, L.Cin_pad >= gemm_f8_min_k(), conv_f8_enabled() && opt("gemm_p3") != 0, up != 0);
    if (L.wdma_bytes) { L.wdma_off = doff; doff += rupz(L.wdma_bytes, 256); }
    if (L.w3_bytes) { L.w3_off = doff; doff += rupz(L.w3_bytes, 256); }
    if (L.wup_bytes) { L.wup_off = doff; doff += rupz(L.wup_bytes, 256); }
    e->convs.push_back(L);
    return (int)e->convs.size() - 1;
  }
  int norm(int C) {
    NormL n; n.C = C;
    n.g_off = woff; woff += rupz((size_t)C * 4, 256);
    n.b_off = woff; woff += rupz((size_t)C * 4, 256);
    e->norms.push_back(n);
    return (int)e->norms.size() - 1;
  }
  void slot(const std::string& key, int kind, int layer, std::vector<int64_t> shape, int co_off = 0, int ci_off = 0) {
    Slot s; s.kind = kind; s.layer = layer; s.co_off = co_off; s.ci_off = ci_off; s.shape = std::move(shape);
    if (kind == SLOT_HOST) {
      size_t n = 1; for (auto d : s.shape) n *= (size_t)d;
      s.host_off = e->hostblob.size();
      e->hostblob.resize(e->hostblob.size() + n, 0.0f);
    }
    e->slots[key] = s;
    e->slot_order.push_back(key);
  }
  // the fp32 tensor of a packed slot is kept on the host as well -> its offset in the host blob
  size_t keep_host(const std::string& key) {
    Slot& s = e->slots[key];
    size_t n = 1; for (auto d : s.shape) n *= (size_t)d;
    s.host_too = true; s.host_off = e->hostblob.size();
    e->hostblob.resize(e->hostblob.size() + n, 0.0f);
    return s.host_off;
  }
  // plain conv / linear layer "<p>.weight"/"<p>.bias"
  int conv_named(const std::string& p, int ntaps, int I, int O, bool bias = true, int ci_off = 0, int Ipad = 0, int up = 0) {
    int id = conv(p, ntaps, Ipad ? Ipad : I, O, 0, up);
    if (ntaps == 9) slot(p + ".weight", SLOT_CONV_W, id, {O, I, 3, 3}, 0, ci_off);
    else slot(p + ".weight", SLOT_CONV_W, id, {O, I}, 0, ci_off);
    if (bias) slot(p + ".bias", SLOT_CONV_B, id, {O});
    return id;
  }
  int norm_named(const std::string& p, int C) {
    int id = norm(C);
    slot(p + ".weight", SLOT_NORM_G, id, {C});
    slot(p + ".bias", SLOT_NORM_B, id, {C});
    return id;
  }
  ResB resnet(const std::string& p, int cin, int cout, int temb_dim) {
    ResB r; r.cin = cin; r.cout = cout;
    r.norm1 = norm_named(p + ".norm1", cin);
    if (temb_dim > 0) {
      // conv1 bias is replaced by a per-variant table (bias + time_emb_proj(silu(emb))): keep host copies
      r.conv1 = conv(p + ".conv1", 9, cin, cout);
      slot(p + ".conv1.weight", SLOT_CONV_W, r.conv1, {cout, cin, 3, 3});
      TembL t; t.cout = cout; t.cout_pad = e->convs[r.conv1].Cout_pad;
      slot(p + ".conv1.bias", SLOT_HOST, -1, {cout}); t.cb_hoff = e->slots[p + ".conv1.bias"].host_off;
      slot(p + ".time_emb_proj.weight", SLOT_HOST, -1, {cout, temb_dim}); t.w_hoff = e->slots[p + ".time_emb_proj.weight"].host_off;
      slot(p + ".time_emb_proj.bias", SLOT_HOST, -1, {cout}); t.b_hoff = e->slots[p + ".time_emb_proj.bias"].host_off;
      e->tembs.push_back(t);
      r.temb = (int)e->tembs.size() - 1;
    } else {
      r.conv1 = conv_named(p + ".conv1", 9, cin, cout);
    }
    r.norm2 = norm_named(p + ".norm2", cout);
    r.conv2 = conv_named(p + ".conv2", 9, cout, cout);
    if (cin != cout) r.sc = conv_named(p + ".conv_shortcut", 1, cin, cout);
    return r;
  }
  VaeAttnB vae_attn(const std::string& p, int C) {
    const int outer = stage;
    stage = SDM_PRECISE_VAE_ATTN_LIN;
    struct Restore { int& s; int v; ~Restore() { s = v; } } restore{stage, outer};
    VaeAttnB a; a.C = C;
    a.gn = norm_named(p + ".group_norm", C);
    a.qkv = conv(p + ".qkv", 1, C, 3 * C);
    const char* nm[3] = {"to_q", "to_k", "to_v"};
    for (int i = 0; i < 3; ++i) {
      slot(p + "." + nm[i] + ".weight", SLOT_CONV_W, a.qkv, {C, C}, i * C);
      slot(p + "." + nm[i] + ".bias", SLOT_CONV_B, a.qkv, {C}, i * C);
    }
    a.out = conv_named(p + ".to_out.0", 1, C, C);
    return a;
  }
  TfB transformer(const std::string& p, int C, int heads, int ctx) {
    const int outer = stage;
    stage = SDM_PRECISE_UNET_TF;
    struct Restore { int& s; int v; ~Restore() { s = v; } } restore{stage, outer};
    TfB t; t.C = C; t.heads = heads;
    t.gn = norm_named(p + ".norm", C);
    t.proj_in = conv_named(p + ".proj_in", 1, C, C);
    const std::string b = p + ".transformer_blocks.0";
    t.ln1 = norm_named(b + ".norm1", C);
    t.ln2 = norm_named(b + ".norm2", C);
    t.ln3 = norm_named(b + ".norm3", C);
    t.qkv1 = conv(b + ".attn1.qkv", 1, C, 3 * C);
    slot(b + ".attn1.to_q.weight", SLOT_CONV_W, t.qkv1, {C, C}, 0);
    slot(b + ".attn1.to_k.weight", SLOT_CONV_W, t.qkv1, {C, C}, C);
    slot(b + ".attn1.to_v.weight", SLOT_CONV_W, t.qkv1, {C, C}, 2 * C);
    t.o1 = conv_named(b + ".attn1.to_out.0", 1, C, C);
    t.q2 = conv_named(b + ".attn2.to_q", 1, C, C, false);
    // softmax(q.k^T * d^-1/2) is evaluated as 2^(q'.k^T - max) with q' = q * d^-1/2 * log2(e): the constant goes into the
    // to_q weights (no bias in these projections), so the attention kernel needs no per-logit multiply
    e->slots[b + ".attn1.to_q.weight"].w_scale = e->slots[b + ".attn2.to_q.weight"].w_scale = 0.125f * SDM_LOG2E;
    // cross-attention K|V: K = W_k (W_aux * z + b_aux) is an affine map of the 3x3 patch of the 4-channel trimap latent z
    // (exact fold): ONE 3x3 conv 16(4 real)->2C with host-folded weights instead of aux_conv_in
    // (4->1024) followed by two 1024->C GEMMs.  to_k / to_v / aux_conv_in are kept on the host and folded in finalize.
    t.kv2 = conv(b + ".attn2.kv_folded", 9, 16, 2 * C);
    slot(b + ".attn2.to_k.weight", SLOT_HOST, -1, {C, ctx}); t.k_hoff = e->slots[b + ".attn2.to_k.weight"].host_off;
    slot(b + ".attn2.to_v.weight", SLOT_HOST, -1, {C, ctx}); t.v_hoff = e->slots[b + ".attn2.to_v.weight"].host_off;
    t.o2 = conv_named(b + ".attn2.to_out.0", 1, C, C);
    // the same cross-attention on the key / value operand that all blocks share (fold_cross_shared): per head the folded K / V weights move into to_q /
    // to_out.0.  Two more C -> C Linears with host-folded weights; to_q / to_out.0 stay packed for the option cross_shared = 0 and keep host copies
    t.q2s = conv(b + ".attn2.q_shared", 1, C, C);
    t.o2s = conv(b + ".attn2.out_shared", 1, C, C);
    t.q_hoff = keep_host(b + ".attn2.to_q.weight");
    t.o_hoff = keep_host(b + ".attn2.to_out.0.weight");
    t.ob_hoff = keep_host(b + ".attn2.to_out.0.bias");
    t.ff1 = conv(b + ".ff.net.0.proj", 1, C, 8 * C, 1);
    slot(b + ".ff.net.0.proj.weight", SLOT_CONV_W, t.ff1, {8 * C, C});
    slot(b + ".ff.net.0.proj.bias", SLOT_CONV_B, t.ff1, {8 * C});
    t.ff2 = conv_named(b + ".ff.net.2", 1, 4 * C, C);
    t.proj_out = conv_named(p + ".proj_out", 1, C, C);
    return t;
  }
};

static std::string S(int i) { return std::to_string(i); }

static void build_model(sdm_ctx* e) {
  Builder B(e);
  const sdm_config& c = e->cfg;
  const int* vc = c.vae_channels;
  const int lc = 4;
  // ---- VAE encoder ----
  B.stage = SDM_PRECISE_VAE_ENC;
  e->enc_conv_in = B.conv_named("vae.encoder.conv_in", 9, 3, vc[0]);
  int cprev = vc[0];
  e->enc_res.resize(4);
  for (int i = 0; i < 4; ++i) {
    for (int j = 0; j < c.vae_layers_per_block; ++j)
      e->enc_res[i].push_back(B.resnet("vae.encoder.down_blocks." + S(i) + ".resnets." + S(j), j == 0 ? cprev : vc[i], vc[i], 0));
    cprev = vc[i];
    if (i < 3) e->enc_down.push_back(B.conv_named("vae.encoder.down_blocks." + S(i) + ".downsamplers.0.conv", 9, vc[i], vc[i]));
  }
  const int cm = vc[3];
  e->enc_mid0 = B.resnet("vae.encoder.mid_block.resnets.0", cm, cm, 0);
  e->enc_attn = B.vae_attn("vae.encoder.mid_block.attentions.0", cm);
  e->enc_mid1 = B.resnet("vae.encoder.mid_block.resnets.1", cm, cm, 0);
  e->enc_norm_out = B.norm_named("vae.encoder.conv_norm_out", cm);
  e->enc_conv_out = B.conv_named("vae.encoder.conv_out", 9, cm, 2 * lc);
  e->quant = B.conv_named("vae.quant_conv", 1, 2 * lc, 2 * lc);
  B.stage = SDM_PRECISE_VAE_DEC;
  e->post_quant = B.conv_named("vae.post_quant_conv", 1, lc, lc);
  // ---- VAE decoder ----
  e->dec_conv_in = B.conv_named("vae.decoder.conv_in", 9, lc, cm);
  e->dec_mid0 = B.resnet("vae.decoder.mid_block.resnets.0", cm, cm, 0);
  e->dec_attn = B.vae_attn("vae.decoder.mid_block.attentions.0", cm);
  e->dec_mid1 = B.resnet("vae.decoder.mid_block.resnets.1", cm, cm, 0);
  e->dec_res.resize(4);
  cprev = vc[3];
  for (int i = 0; i < 4; ++i) {
    const int co = vc[3 - i];
    for (int j = 0; j < c.vae_layers_per_block + 1; ++j)
      e->dec_res[i].push_back(B.resnet("vae.decoder.up_blocks." + S(i) + ".resnets." + S(j), j == 0 ? cprev : co, co, 0));
    cprev = co;
    if (i < 3) e->dec_up.push_back(B.conv_named("vae.decoder.up_blocks." + S(i) + ".upsamplers.0.conv", 9, co, co, true, 0, 0, 1));
  }
  e->dec_norm_out = B.norm_named("vae.decoder.conv_norm_out", vc[0]);
  e->dec_conv_out = B.conv_named("vae.decoder.conv_out", 9, vc[0], 3);
  // ---- U-Net ----
  B.stage = SDM_PRECISE_UNET_RES;
  const int* uc = c.unet_channels;
  const int te = uc[0] * 4, ctx = c.cross_attention_dim;
  e->u_conv_in = B.conv_named("unet.conv_in", 9, c.unet_in_channels, uc[0]);
  // aux_conv_in (4->ctx, utils.py:33-41) only ever feeds the cross-attention K/V projections: folded into them (see transformer())
  e->u_aux = -1;
  B.slot("unet.aux_conv_in.weight", SLOT_HOST, -1, {ctx, 4, 3, 3}); e->h_auxw = e->slots["unet.aux_conv_in.weight"].host_off;
  B.slot("unet.aux_conv_in.bias", SLOT_HOST, -1, {ctx}); e->h_auxb = e->slots["unet.aux_conv_in.bias"].host_off;
  B.slot("unet.time_embedding.linear_1.weight", SLOT_HOST, -1, {te, uc[0]}); e->h_time1w = e->slots["unet.time_embedding.linear_1.weight"].host_off;
  B.slot("unet.time_embedding.linear_1.bias", SLOT_HOST, -1, {te}); e->h_time1b = e->slots["unet.time_embedding.linear_1.bias"].host_off;
  B.slot("unet.time_embedding.linear_2.weight", SLOT_HOST, -1, {te, te}); e->h_time2w = e->slots["unet.time_embedding.linear_2.weight"].host_off;
  B.slot("unet.time_embedding.linear_2.bias", SLOT_HOST, -1, {te}); e->h_time2b = e->slots["unet.time_embedding.linear_2.bias"].host_off;
  const int bd = c.bbox_embeddings_input_dim;
  B.slot("unet.bbox_embedding.linear_1.weight", SLOT_HOST, -1, {te, bd}); e->h_bbox1w = e->slots["unet.bbox_embedding.linear_1.weight"].host_off;
  B.slot("unet.bbox_embedding.linear_1.bias", SLOT_HOST, -1, {te}); e->h_bbox1b = e->slots["unet.bbox_embedding.linear_1.bias"].host_off;
  B.slot("unet.bbox_embedding.linear_2.weight", SLOT_HOST, -1, {te, te}); e->h_bbox2w = e->slots["unet.bbox_embedding.linear_2.weight"].host_off;
  B.slot("unet.bbox_embedding.linear_2.bias", SLOT_HOST, -1, {te}); e->h_bbox2b = e->slots["unet.bbox_embedding.linear_2.bias"].host_off;
  // point prompts (replace.py:198,446-450): TimestepEmbedding(point_embeddings_input_dim -> 1280), host-side like bbox_embedding
  const int pd = c.point_embeddings_input_dim;
  B.slot("unet.point_embedding.linear_1.weight", SLOT_HOST, -1, {te, pd}); e->h_point1w = e->slots["unet.point_embedding.linear_1.weight"].host_off;
  B.slot("unet.point_embedding.linear_1.bias", SLOT_HOST, -1, {te}); e->h_point1b = e->slots["unet.point_embedding.linear_1.bias"].host_off;
  B.slot("unet.point_embedding.linear_2.weight", SLOT_HOST, -1, {te, te}); e->h_point2w = e->slots["unet.point_embedding.linear_2.weight"].host_off;
  B.slot("unet.point_embedding.linear_2.bias", SLOT_HOST, -1, {te}); e->h_point2b = e->slots["unet.point_embedding.linear_2.bias"].host_off;
  e->u_down_res.resize(4); e->u_down_tf.resize(4);
  cprev = uc[0];
  for (int i = 0; i < 4; ++i) {
    for (int j = 0; j < c.unet_layers_per_block; ++j) {
      e->u_down_res[i].push_back(B.resnet("unet.down_blocks." + S(i) + ".resnets." + S(j), j == 0 ? cprev : uc[i], uc[i], te));
      if (i < 3) e->u_down_tf[i].push_back(B.transformer("unet.down_blocks." + S(i) + ".attentions." + S(j), uc[i], c.unet_heads[i], ctx));
    }
    cprev = uc[i];
    if (i < 3) e->u_down_ds.push_back(B.conv_named("unet.down_blocks." + S(i) + ".downsamplers.0.conv", 9, uc[i], uc[i]));
  }
  e->u_mid0 = B.resnet("unet.mid_block.resnets.0", uc[3], uc[3], te);
  e->u_midtf = B.transformer("unet.mid_block.attentions.0", uc[3], c.unet_heads[3], ctx);
  e->u_mid1 = B.resnet("unet.mid_block.resnets.1", uc[3], uc[3], te);
  e->u_up_res.resize(4); e->u_up_tf.resize(4);
  int output_channel = uc[3];
  const int nl = c.unet_layers_per_block + 1;
  for (int i = 0; i < 4; ++i) {
    const int prev_out = output_channel;
    output_channel = uc[3 - i];
    const int input_channel = uc[3 - std::min(i + 1, 3)];
    for (int j = 0; j < nl; ++j) {
      const int res_skip = (j == nl - 1) ? input_channel : output_channel;
      const int resnet_in = (j == 0) ? prev_out : output_channel;
      e->u_up_res[i].push_back(B.resnet("unet.up_blocks." + S(i) + ".resnets." + S(j), resnet_in + res_skip, output_channel, te));
      if (i > 0) e->u_up_tf[i].push_back(B.transformer("unet.up_blocks." + S(i) + ".attentions." + S(j), output_channel, c.unet_heads[3 - i], ctx));
    }
    if (i < 3) e->u_up_us.push_back(B.conv_named("unet.up_blocks." + S(i) + ".upsamplers.0.conv", 9, output_channel, output_channel, true, 0, 0, 1));
  }
  e->u_norm_out = B.norm_named("unet.conv_norm_out", uc[0]);
  e->u_conv_out = B.conv_named("unet.conv_out", 9, uc[0], c.unet_out_channels);
  e->canon_bytes = B.woff;
  e->warena_bytes = B.woff + B.doff;
}

// ------------------------------------------------------------------------------------------------
// arena
// ------------------------------------------------------------------------------------------------
static const size_t kAsideOff = (size_t)1 << 62;      // T::off (and soff / cm_off) of a buffer outside the arena: tfree leaves it alone

static void arena_diverged(sdm_ctx* e, const char* fmt, size_t i, size_t a, size_t b) {
  if (e->adiverged) return;
  char buf[256];
  snprintf(buf, sizeof(buf), fmt, i, a, b);
  e->adiverged = true; e->adiv_msg = buf;
}

// launch pass after a divergence: a buffer of its own (the arena is only known to hold what the sizing pass placed in it).  Should even this
// allocation fail, the null pointer faults the kernel that gets it instead of letting it write past the arena.
static T talloc_aside(sdm_ctx* e, T t) {
  void* p = nullptr;
  if (dev_malloc(&p, t.bytes) != 0) p = nullptr;
  e->aside.push_back(p);
  t.off = kAsideOff; t.p = p;
  return t;
}

static T talloc(sdm_ctx* e, int N, int H, int W, int C, int f32) {
  T t; t.N = N; t.H = H; t.W = W; t.C = C; t.f32 = f32;
  t.bytes = rupz((f32 == kFmtP3 ? p3_rows_pad((size_t)N * H * W) : (size_t)N * H * W) * C * fmt_bytes(f32), 256);      // (P3 planes are blocked: rows padded to 32)
  if (e->dry) e->atrace.push_back(t.bytes);
  else {
    const size_t i = e->atrace_i++;
    const size_t want = i < e->atrace.size() ? e->atrace[i] : 0;
    if (want != t.bytes) arena_diverged(e, "allocation %zu: %zu bytes in the sizing pass, %zu in the launch pass", i, want, t.bytes);
    if (e->adiverged) return talloc_aside(e, t);
  }
  // first fit in the free list
  for (auto it = e->freelist.begin(); it != e->freelist.end(); ++it) {
    if (it->second >= t.bytes) {
      t.off = it->first;
      const size_t rem = it->second - t.bytes;
      e->freelist.erase(it);
      if (rem) e->freelist[t.off + t.bytes] = rem;
      t.p = e->dry ? nullptr : e->arena + t.off;
      return t;
    }
  }
  if (!e->dry && e->arena_top + t.bytes > e->arena_bytes) {      // the same sizes in the same order, yet past the end (frees that differ)
    arena_diverged(e, "allocation %zu: ends at byte %zu of an arena of %zu", e->atrace_i - 1, e->arena_top + t.bytes, e->arena_bytes);
    return talloc_aside(e, t);
  }
  t.off = e->arena_top;
  e->arena_top += t.bytes;
  e->peak = std::max(e->peak, e->arena_top);
  t.p = e->dry ? nullptr : e->arena + t.off;
  return t;
}

static void tfree_raw(sdm_ctx* e, size_t off, size_t sz);
static void tfree(sdm_ctx* e, T& t) {
  if (!t.bytes) return;
  if (t.sbytes) { tfree_raw(e, t.soff, t.sbytes); t.sbytes = 0; t.stats = nullptr; }
  if (t.cm_bytes) { tfree_raw(e, t.cm_off, t.cm_bytes); t.cm_bytes = 0; t.cmask = nullptr; }
  tfree_raw(e, t.off, t.bytes);
  t.bytes = 0; t.p = nullptr;
}
static void tfree_raw(sdm_ctx* e, size_t off, size_t sz) {
  if (off >= kAsideOff) return;                  // outside the arena: released by arena_pass_end
  auto nx = e->freelist.lower_bound(off);
  if (nx != e->freelist.begin()) {
    auto pv = std::prev(nx);
    if (pv->first + pv->second == off) { off = pv->first; sz += pv->second; e->freelist.erase(pv); }
  }
  nx = e->freelist.lower_bound(off + sz);
  if (nx != e->freelist.end() && nx->first == off + sz) { sz += nx->second; e->freelist.erase(nx); }
  if (off + sz == e->arena_top) e->arena_top = off;
  else e->freelist[off] = sz;
}

// mark t so that the conv producing it also emits the GroupNorm statistics of its consumer (op_conv allocates the
// partial-row buffer once the tile configuration, hence the number of rows, is known)
static int tstats(sdm_ctx* e, T& t) { (void)e; t.want_stats = true; return 0; }

static void arena_reset(sdm_ctx* e) { e->freelist.clear(); e->arena_top = 0; }

static void arena_release_aside(sdm_ctx* e) {
  if (e->aside.empty()) return;
  dev_sync(e->stream);                           // (kernels of the pass may still use them)
  for (void* p : e->aside) if (p) dev_free(p);
  e->aside.clear();
}

// start of either pass of arena_two_pass: pass 0 sizes the arena without memory, pass 1 launches in it
static void arena_pass_begin(sdm_ctx* e, int pass) {
  arena_release_aside(e);                        // (left behind by a launch pass that ended early)
  e->dry = (pass == 0);
  arena_reset(e);
  if (pass == 0) { e->peak = 0; e->atrace.clear(); }
  e->atrace_i = 0; e->adiverged = false; e->adiv_msg.clear();
}

// end of the launch pass (rc: its own status, which takes precedence): an allocation that differed from the sizing pass is an error
static int arena_pass_end(sdm_ctx* e, int rc) {
  e->dry = false;
  arena_release_aside(e);
  if (rc) return rc;
  if (!e->adiverged && e->atrace_i != e->atrace.size())
    arena_diverged(e, "allocation %zu: the sizing pass made %zu allocations, the launch pass %zu", e->atrace_i, e->atrace.size(), e->atrace_i);
  if (e->adiverged) SDM_FAIL(e, SDM_ERR_ARENA, "activation arena: the launch pass diverged from the sizing pass at %s", e->adiv_msg.c_str());
  return 0;
}

// replaces the arena by one of `bytes`, once the kernels that still use the old one are done
static int arena_grow(sdm_ctx* e, size_t bytes) {
  if (e->arena) { SDM_CHECK_DEV(e, dev_sync(e->stream)); dev_free(e->arena); e->arena = nullptr; e->arena_bytes = 0; }
  void* p = nullptr;
  if (dev_malloc(&p, bytes) != 0) SDM_FAIL(e, SDM_ERR_NOMEM, "cannot allocate %zu bytes of activation arena", bytes);
  e->arena = (unsigned char*)p; e->arena_bytes = bytes;
  return 0;
}

// The one two-pass loop: body() runs twice, its tallocs sized without memory first (e->dry), then placed in an arena of at least `floor` bytes
// that holds their peak.  mark_ev0: the launch pass starts at ev0 (sdm_last_forward_ms).  Every error return goes through arena_pass_end.
template <typename F>
static int arena_two_pass(sdm_ctx* e, size_t floor, bool mark_ev0, F body) {
  for (int pass = 0; pass < 2; ++pass) {
    arena_pass_begin(e, pass);
    int rc = 0;
    if (pass == 1) {
      if (e->peak > e->arena_bytes) rc = arena_grow(e, std::max(e->peak, floor));
#ifndef SDM_EMU
      if (!rc && mark_ev0) (void)hipEventRecord(e->ev0, (hipStream_t)e->stream);
#else
      (void)mark_ev0;
#endif
    }
    if (!rc) rc = body();
    if (rc || pass == 1) return arena_pass_end(e, rc);
  }
  return 0;
}

// ------------------------------------------------------------------------------------------------
// profiling helpers
// ------------------------------------------------------------------------------------------------
static void prof_begin(sdm_ctx* e, const char* name, double flops, double bytes, const std::string& desc = std::string()) {
  if (!e->prof_on || e->dry) return;
  ProfRec r; r.name = name; r.desc = desc; r.flops = flops; r.bytes = bytes;
#ifndef SDM_EMU
  (void)hipEventCreate(&r.e0); (void)hipEventCreate(&r.e1);
  (void)hipEventRecord(r.e0, (hipStream_t)e->stream);
#endif
  e->prof.push_back(r);
}
static void prof_end(sdm_ctx* e) {
  if (!e->prof_on || e->dry) return;
#ifndef SDM_EMU
  (void)hipEventRecord(e->prof.back().e1, (hipStream_t)e->stream);
#endif
}

// ------------------------------------------------------------------------------------------------
// operators
// ------------------------------------------------------------------------------------------------
struct ConvArgs {
  const T* in0 = nullptr; const T* in1 = nullptr;
  int up = 0, stride = 1, pad_mode = 0;
  T* out = nullptr;            // pre-allocated output (shape/dtype/C define the store)
  int out_ch_off = 0, cout_valid = -1;
  int lo_cols = -1;            // plane outputs (T::f32 2 / 3): output channels that need the low-part plane (-1: all)
  const T* res = nullptr;
  float out_scale = 1.0f;
  const float* bias_override = nullptr; const int* bias_sel = nullptr;
  int force_cfg = -1;
  const float* gn_scale = nullptr; const float* gn_shift = nullptr; int gn_silu = 0;   // fused GroupNorm apply (tile cfg 0 only)
};

// The shape part of ConvParams - all that conv_pick_cfg and conv_cfg_ok read.  op_conv and the fuse test of gn_conv both fill it here, so the tile
// gn_conv asks about is the tile op_conv would pick.
static void conv_shape_params(ConvParams& p, const ConvL& L, const T& in0, const T* in1, const T& out, int stride) {
  p.C0 = in0.C; p.C1 = in1 ? in1->C : 0; p.in_f32 = in0.f32;
  p.N = in0.N; p.Hin = in0.H; p.Win = in0.W;
  p.Hout = out.H; p.Wout = out.W;
  p.M = out.rows();
  p.Cout_pad = L.Cout_pad;
  p.f8_hint = (L.f8 && L.w_dma && p.in_f32 && L.ntaps == 9 && stride == 1) ? 1 : 0;
}

// Upsample2D on the phase path (k_gemm.h, UP): the layer keeps phase matrices (ConvL::wup), fp32 in and out, nothing fused but bias and statistics
static bool conv_up_phase_ok(const ConvL& L, const ConvArgs& a) {
  if (!L.wup_bytes || a.up != 1 || a.stride != 1 || a.pad_mode != 0 || a.in1 || a.res || a.bias_sel || a.bias_override || a.gn_scale || a.force_cfg >= 0) return false;
  if (a.in0->f32 != 1 || a.out->f32 != 1 || a.out_scale != 1.0f || a.out_ch_off != 0 || a.in0->C != L.Cin_pad || a.out->C % 4) return false;
  const int nv = a.cout_valid >= 0 ? a.cout_valid : std::min(L.Cout_pad, a.out->C);
  if (nv % 32 || nv > L.Cout_pad) return false;
  if (!up_phase_wins(a.in0->N, a.in0->H, a.in0->W, L.Cout_pad)) return false;
  const size_t rows = (size_t)a.in0->N * (a.in0->H + 2) * (a.in0->W + 2);
  // one buffer descriptor over each operand plane, one over the output rows of a 256-row tile: both short of the offset that marks a dropped access
  const size_t tile_out = (size_t)2 * (256 / (a.in0->W + 2) + 2) * 2 * a.in0->W * a.out->C * 4;
  return p3_rows_pad(rows) * (size_t)L.Cin_pad * 2 < SDM_BUF_INVALID && tile_out < SDM_BUF_INVALID && rows < ((size_t)1 << 31);
}
// test option dbg_stats_poison: the partial rows of `t` start as NaN (launch pass only; nothing is allocated)
static int stats_poison(sdm_ctx* e, const T& t) {
  if (e->dry || !t.stats || !opt("dbg_stats_poison")) return 0;
  SDM_CHECK_DEV(e, dev_memset(t.stats, 0xFF, (size_t)t.N * t.srows * t.C * 2 * 4, e->stream));
  return 0;
}

static int op_conv_up_phase(sdm_ctx* e, const ConvL& L, const ConvArgs& a) {
  const T& in = *a.in0;
  T* out = a.out;
  T xp = talloc(e, in.N, in.H + 2, in.W + 2, in.C, kFmtP3);
  GemmP3Params p;
  memset(&p, 0, sizeof(p));
  p.M = xp.rows(); p.K = L.Cin_pad; p.rows_per_img = (in.H + 2) * (in.W + 2);
  p.up_H = in.H; p.up_W = in.W;
  p.a_hi = (const half_t*)xp.p; p.a_xl = (const unsigned char*)xp.p + p3_rows_pad((size_t)p.M) * p.K * 2;
  p.w = L.wup; p.N = L.Cout_pad; p.bias = L.b;
  p.out = out->p; p.ldo = out->C; p.n_valid = a.cout_valid >= 0 ? a.cout_valid : std::min(L.Cout_pad, out->C);
  p.sa = 127 - 11; p.sb = 127 - L.up_exp;
  const int bm = gemm_p3_pick_bm(p.M, p.N, p.rows_per_img, 4);
  const int epi = out->want_stats ? 4 : 0;
  if (epi == 4) {
    out->srows = sdm_cdiv(p.rows_per_img, bm) * 8;                  // partial row (M tile, phase, wave row)
    T sb = talloc(e, 1, 1, 1, (int)((size_t)in.N * out->srows * out->C * 2), 1);
    out->soff = sb.off; out->sbytes = sb.bytes; out->stats = (float*)sb.p;
    p.stats = out->stats;
  }
  if (e->dry) { tfree(e, xp); return 0; }
  if (epi == 4) TRY(stats_poison(e, *out));
  char d[256];
  d[0] = 0;
  if (e->prof_on) snprintf(d, sizeof(d), "%s N=%d H=%d W=%d C=%d bordered grid", L.name.c_str(), in.N, in.H, in.W, in.C);
  prof_begin(e, "to_p3", 0, (double)in.rows() * in.C * 4 + (double)xp.rows() * in.C * 3, d);
  const long units = ((xp.rows() + 31) / 32) * (in.C / 32);
  SDM_LAUNCH(to_p3_pad_kernel, dim3((unsigned)std::min<long>((units + 3) / 4, 1 << 20)), dim3(256), 0, e->stream, (const float*)in.p, (unsigned char*)xp.p, xp.rows(), in.C,
             in.H, in.W);
  prof_end(e);
  // EXECUTED flops: four taps per output pixel (the 3x3 form of the same layer counts nine)
  const double flops = 2.0 * (double)out->rows() * L.O * L.I * 4;
  const double bytes = (double)xp.rows() * p.K * 3 + (double)out->rows() * p.n_valid * 4 + (double)16 * p.K * p.N * 4;
  if (e->prof_on) {
    snprintf(d, sizeof(d), "%s N=%d Hout=%d Wout=%d Cin=%d Cout=%d up=1 phases epi=%d bm=%d", L.name.c_str(), in.N, out->H, out->W, L.Cin_pad, L.O, epi, bm);
    prof_begin(e, "conv_up_phase", flops, bytes, d);
  } else {
    prof_begin(e, "conv", flops, bytes);
  }
  count_kernel("conv_up_phase");
  launch_gemm_p3_up(p, epi, bm, e->stream);
#ifndef SDM_EMU
  { const hipError_t le = hipGetLastError(); if (le != hipSuccess) SDM_FAIL(e, SDM_ERR_HIP, "conv %s: launch failed: %s", L.name.c_str(), hipGetErrorString(le)); }
#endif
  prof_end(e);
  tfree(e, xp);
  return 0;
}

static int op_conv(sdm_ctx* e, const ConvL& L, const ConvArgs& a) {
  if (conv_up_phase_ok(L, a)) return op_conv_up_phase(e, L, a);
  ConvParams p;
  memset(&p, 0, sizeof(p));
  conv_shape_params(p, L, *a.in0, a.in1, *a.out, a.stride);
  p.in0 = a.in0->p;
  if (a.in1) p.in1 = a.in1->p;
  p.up = a.up;
  p.pad_t = p.pad_l = (a.pad_mode == 0) ? 1 : 0;
  p.w = L.w; p.bias = a.bias_override ? a.bias_override : L.b; p.bias_sel = a.bias_sel;
  p.out = a.out->p; p.out_f32 = a.out->f32; p.Cout_store = a.out->C;
  p.out_lo_off = (size_t)a.out->rows() * a.out->C;
  p.lo_cols = a.lo_cols >= 0 ? a.lo_cols : (1 << 30);
  p.acc_scale = 1.0f;
  if (L.split) {
    if (!p.in_f32) SDM_FAIL(e, SDM_ERR_INVALID, "conv %s: split-precision layers take fp32 activations", L.name.c_str());
    p.w_lo = L.w_lo; p.acc_scale = ldexpf(1.0f, -L.w_exp);
  }
  const int nout = L.geglu ? L.Cout_pad / 2 : L.Cout_pad;
  p.Cout_valid = a.cout_valid >= 0 ? a.cout_valid : std::min(nout, a.out->C - a.out_ch_off);
  p.out_ch_off = a.out_ch_off;
  if (a.res) { p.res = a.res->p; p.res_f32 = a.res->f32; p.res_C = a.res->C; }
  p.epi = L.geglu; p.out_scale = a.out_scale;
  p.epi_mode = conv_epi_mode();
  p.xtile = conv_xtile_enabled() ? 1 : 0;
  p.gn_scale = a.gn_scale; p.gn_shift = a.gn_shift; p.gn_silu = a.gn_silu;
  // the F8 3x3 kernel addresses both tables through ONE buffer descriptor: scale | shift are the two halves of one scratch tensor (gn_scale_shift)
  if (!e->dry && a.gn_scale && a.gn_shift != a.gn_scale + (size_t)a.in0->N * (a.in0->C + (a.in1 ? a.in1->C : 0)))
    SDM_FAIL(e, SDM_ERR_STATE, "fused GroupNorm: shift table is not scale + N * C");
  if ((long)a.in0->rows() >= (1L << 31) || p.M >= (1L << 31)) SDM_FAIL(e, SDM_ERR_INVALID, "conv %s: tensor too large for 32-bit pixel indices", L.name.c_str());
  {   // 3x3: per-tile descriptors span only the rows of the tile's halo (k_conv.h band0), so an image may exceed 4 GB; what
      // stays 32-bit is the byte offset inside that band
    const size_t es_in = p.in_f32 ? 4 : 2;
    if (L.ntaps == 9 && (size_t)40 * p.Win * (size_t)std::max(p.C0, p.C1) * es_in >= 0xFFFF0000ull)
      SDM_FAIL(e, SDM_ERR_INVALID, "conv %s: a %d-pixel-wide row band of the operand exceeds a buffer descriptor", L.name.c_str(), p.Win);
  }
  if (p.C0 + p.C1 != L.Cin_pad) SDM_FAIL(e, SDM_ERR_INVALID, "conv %s: input channels %d+%d != %d", L.name.c_str(), p.C0, p.C1, L.Cin_pad);
  if (a.in1 && a.in1->f32 != a.in0->f32) SDM_FAIL(e, SDM_ERR_INVALID, "conv %s: concat sources differ in dtype", L.name.c_str());
  int cfg = a.force_cfg >= 0 ? a.force_cfg : conv_pick_cfg(L.ntaps, a.stride, p);
  if (cfg < 0 || cfg >= conv_num_cfgs(L.ntaps, a.stride) || !conv_cfg_ok(conv_cfg_table(L.ntaps, a.stride)[cfg], p))
    SDM_FAIL(e, SDM_ERR_INVALID, "conv %s: no tile configuration for Cin=%d+%d (cfg %d)", L.name.c_str(), p.C0, p.C1, cfg);
  if (a.gn_scale && !(L.ntaps == 9 && a.stride == 1 && (cfg == 0 || cfg == 4 || cfg == 5) && p.C0 + p.C1 <= 1024))
    SDM_FAIL(e, SDM_ERR_INVALID, "conv %s: fused GroupNorm requested for an unsupported tile configuration", L.name.c_str());
  // weights by LDS-DMA (256x128 tile, 3x3 stride 1): the layer keeps a stage-ordered copy of its weights for that kernel
  const bool dma_off = opt("conv_dma") == 0;      // A/B option
  if (!dma_off && L.ntaps == 9 && a.stride == 1 && cfg == 0 && L.w_dma && (!L.split || p.in_f32)) p.w_dma = L.w_dma;
  {   // producer / consumer form of the split-precision DMA kernel (k_conv.h, PC): the option conv_pc = 0 / 1 forces it off / on
    const int pc_opt = opt("conv_pc"), pc_min_cin = opt("conv_pc_min_cin");
    if (p.w_dma && L.split) p.pc = pc_opt >= 0 ? (pc_opt == 1) : (L.Cin_pad >= pc_min_cin);
    if (p.w_dma && L.f8) {
      // the fp8-residual kernel stages 32-channel chunks: a channel concat that does not split on a chunk boundary takes the
      // register-staged split kernel (K16 weights) instead
      if (p.C1 > 0 && (p.C0 % 32)) { p.w_dma = nullptr; p.pc = 0; }
      else p.f8 = 1;
    }
    if (L.ntaps == 1 && L.f8 && L.w_dma && cfg == 4 && p.in_f32 && gemm_f8_enabled()) { p.w_dma = L.w_dma; p.f8 = 1; }
    // F8 launches: x_lo8 * w8 = (x_lo * 2^11)(w * 2^e8), x8 * w_lo8 = x (w_lo * 2^e8 * 2^11), e8 = the layer's own e4m3 scale: both residual
    // sums are 2^(11 + e8) too large (E8M0 operand scales); the fp16 high parts are packed unscaled -> the accumulators are in the
    // output's unit (acc_scale 1; the K16 hi | lo copy of the same layer, used by the other kernels, keeps 2^-w_exp)
    if (p.f8) { p.f8_sa = 127 - 11; p.f8_sb = 127 - L.f8_exp; p.acc_scale = 1.0f; }
  }
  // split-K (register-staged kernels only): partial sums into an arena workspace, finished by splitk_reduce_kernel
  int ksplit = 1;
  if (!p.w_dma && !L.geglu && p.out_f32 <= 1 && (L.ntaps == 9 || p.M == (long)p.N * p.Hout * p.Wout)) ksplit = conv_pick_ksplit(L.ntaps, a.stride, cfg, p);
  T ws; ws.bytes = 0;
  const int sk_bpi = sdm_cdiv(p.Hout * p.Wout, kSplitKRows);
  if (ksplit > 1 && (size_t)ksplit * p.M * p.Cout_pad >= (1ull << 31)) ksplit = 1;
  if (a.out->want_stats) {
    if (L.geglu || a.out_ch_off || p.out_f32 >= 2) SDM_FAIL(e, SDM_ERR_INVALID, "conv %s: fused statistics unsupported with this epilogue", L.name.c_str());
    const ConvCfgInfo& ci = conv_cfg_table(L.ntaps, a.stride)[cfg];
    const long tiles = (L.ntaps == 9) ? (long)sdm_cdiv(p.Hout, ci.TH) * sdm_cdiv(p.Wout, ci.TW)
                                      : ((long)p.Hout * p.Wout + ci.TH * ci.TW - 1) / (ci.TH * ci.TW);
    // split-K: the statistics come from the reduce kernel, one partial row per kSplitKRows rows of an image
    a.out->srows = ksplit > 1 ? sk_bpi : (int)(tiles * ci.WM);
    T sb = talloc(e, 1, 1, 1, (int)((size_t)p.N * a.out->srows * a.out->C * 2), 1);
    a.out->soff = sb.off; a.out->sbytes = sb.bytes; a.out->stats = (float*)sb.p;
    p.stats = a.out->stats;
  }
  if (ksplit > 1) ws = talloc(e, 1, 1, 1, (int)((size_t)ksplit * p.M * p.Cout_pad), 1);
  // class plane of a piecewise-constant batch (the trimap images of the VAE encoder, k_misc.h cmask_*): eroded through this conv's window; on the
  // F8 kernel's full-tile fp32 path the output tiles that lie inside one region are not multiplied - one representative per (image, class) is,
  // and const_tile_fill_kernel copies it (and its statistics) into the others.  (cm_bytes, not the pointer, drives every decision: the dry pass
  // has no pointers and must allocate the same way.)
  // (no plane behind the last level that can leave tiles out: resolutions only shrink from here, up-sampling convs do not propagate)
  const bool cm_prop = a.in0->cm_bytes != 0 && !a.in1 && L.ntaps == 9 && !a.up && opt("trimap_skip") != 0 && p.Hout >= opt("trimap_skip_min_rows");
  bool cm_skip = false;
  T cm_flag, cm_rep;
  const int cm_tiles = sdm_cdiv(p.Hout, 8) * sdm_cdiv(p.Wout, 32);
  if (cm_prop) {
    T mb = talloc(e, 1, 1, 1, (int)(((size_t)p.N * p.Hout * p.Wout + 3) / 4), 1);
    a.out->cmask = (unsigned char*)mb.p; a.out->cm_off = mb.off; a.out->cm_bytes = mb.bytes; a.out->cm_n0 = a.in0->cm_n0;
    cm_skip = p.f8 && p.w_dma && cfg == 0 && a.stride == 1 && p.Hout % 8 == 0 && p.Wout % 32 == 0 && p.out_f32 == 1 && !L.geglu && p.out_scale == 1.0f &&
              p.Cout_valid == p.Cout_pad && p.Cout_pad % 128 == 0 && p.Cout_store == p.Cout_pad && p.out_ch_off == 0 && (!p.res || p.res_f32) && ksplit == 1;
    if (cm_skip) {
      cm_flag = talloc(e, 1, 1, 1, (p.N * cm_tiles + 3) / 4, 1);
      cm_rep = talloc(e, 1, 1, 1, p.N * 8, 1);
      p.tile_flag = (const unsigned char*)cm_flag.p; p.tile_rep = (const int*)cm_rep.p;
    }
  }
  if (e->dry) { if (ksplit > 1) tfree(e, ws); if (cm_skip) { tfree(e, cm_rep); tfree(e, cm_flag); } return 0; }
  if (p.stats) TRY(stats_poison(e, *a.out));
  const double flops = 2.0 * (double)p.M * L.O * L.I * L.ntaps;
  const double bytes = (double)a.in0->rows() * L.Cin_pad * (p.in_f32 ? 4 : 2) + (double)p.M * p.Cout_valid * (p.out_f32 ? 4 : 2) +
                       (double)L.Cin_pad * L.ntaps * L.Cout_pad * 2 + (a.res ? (double)p.M * p.Cout_valid * (p.res_f32 ? 4 : 2) : 0.0);
  if (e->prof_on) {
    char d[256];
    snprintf(d, sizeof(d), "%s N=%d Hout=%d Wout=%d Cin=%d Cout=%d s=%d up=%d f32in=%d cfg=%d", L.name.c_str(), p.N, p.Hout, p.Wout, L.Cin_pad, L.O, a.stride,
             a.up, p.in_f32, cfg);
    // thin convs (<= 16 real input or output channels: conv_in/conv_out, latent convs, folded cross-attn K|V) are HBM-bound
    // (SURVEY.md 2.2 "thin convs"); everything else is MFMA-bound
    const bool thin = (L.ntaps == 9) && (L.I <= 16 || L.O <= 16);
    prof_begin(e, L.ntaps == 9 ? (thin ? "conv3x3_thin" : "conv3x3_mfma") : "gemm_mfma", flops, bytes, d);
  } else {
    prof_begin(e, "conv", flops, bytes);
  }
  if (L.ntaps == 9 && (L.I <= 16 || L.O <= 16)) count_kernel("conv3x3_thin");
  int rc = 0;
  // GEMMs that emit per-image GroupNorm statistics for a batch: row tiles aligned to images inside ONE launch
  if (L.ntaps == 1 && p.stats && p.N > 1) p.rows_per_img = p.Hout * p.Wout;
  if (cm_prop) {
    const int n0 = a.in0->cm_n0;
    if (cm_skip) {
      SDM_CHECK_DEV(e, dev_memset(cm_rep.p, 0x7f, (size_t)p.N * 8 * 4, e->stream));
      if (n0 > 0) SDM_CHECK_DEV(e, dev_memset(cm_flag.p, 0, (size_t)n0 * cm_tiles, e->stream));
    }
    SDM_LAUNCH(cmask_conv_kernel, dim3((unsigned)cm_tiles, (unsigned)(p.N - n0), 1), dim3(256), 0, e->stream, (const unsigned char*)a.in0->cmask, a.in0->H, a.in0->W, a.out->cmask,
               p.Hout, p.Wout, a.stride, p.pad_t, p.pad_l, cm_skip ? (unsigned char*)cm_flag.p : (unsigned char*)nullptr, cm_skip ? (int*)cm_rep.p : (int*)nullptr, n0);
    if (cm_skip) count_kernel("conv3x3_f8_const_tiles");
  }
  if (ksplit > 1) {
    count_kernel(L.ntaps == 9 ? "conv3x3_splitk" : "gemm_splitk");
    rc = launch_conv_splitk(L.ntaps, a.stride, cfg, p, ksplit, (float*)ws.p, e->stream);
    tfree(e, ws);
  } else {
    rc = launch_conv(L.ntaps, a.stride, cfg, p, e->stream);
  }
  if (cm_skip) {
    if (rc == 0) SDM_LAUNCH(const_tile_fill_kernel, dim3((unsigned)cm_tiles, (unsigned)(p.N - a.in0->cm_n0), 1), dim3(256), 0, e->stream, (float*)p.out, p.Cout_store, p.Hout, p.Wout,
                            p.tile_flag, p.tile_rep, p.stats, 2, a.in0->cm_n0);
    tfree(e, cm_rep); tfree(e, cm_flag);
  }
  if (rc != 0) SDM_FAIL(e, SDM_ERR_INVALID, "conv %s: bad cfg", L.name.c_str());
#ifndef SDM_EMU
  { const hipError_t le = hipGetLastError(); if (le != hipSuccess) SDM_FAIL(e, SDM_ERR_HIP, "conv %s: launch failed: %s", L.name.c_str(), hipGetErrorString(le)); }
#endif
  prof_end(e);
  return 0;
}

// Launch geometry of gn_stats_kernel and gn_apply_kernel (k_norm.h): a thread owns 8 channels, `slots` pixels run side by side in a block, a block walks
// ppb pixels of one image (a multiple of slots), nb blocks per image.
struct GnGeometry { int threads, ppb, nb, slots; };
static GnGeometry gn_geometry(int C, int N, int HW) {
  GnGeometry g;
  const int CV = C / 8;
  g.slots = std::max(1, 256 / CV);
  g.threads = rup(CV * g.slots, 64);
  g.ppb = rup(std::max(g.slots * 8, sdm_cdiv(HW, 2048 / std::max(1, N))), g.slots);
  g.nb = sdm_cdiv(HW, g.ppb);
  return g;
}

// GroupNorm statistics -> per-(image, channel) scale = rstd*gamma and shift = beta - mean*rstd*gamma.
// scratch layout: [N][max(groups,C)][2] doubles (sums) | scale [N][C] floats | shift [N][C] floats.  The caller frees `scratch`.
static int gn_scale_shift(sdm_ctx* e, const void* in0, const void* in1, int C0, int C1, int in_f32, int N, int HW, int groups, const float* gamma,
                          const float* beta, float eps, const float* st0, int rows0, const float* st1, int rows1, bool have_stats, T* scratch,
                          float** scale_out, float** shift_out) {
  const int C = C0 + C1;
  if (C % 8 || (C / groups) * groups != C || C0 % 8) SDM_FAIL(e, SDM_ERR_INVALID, "groupnorm: bad channels %d+%d", C0, C1);
  const size_t sum_bytes = (size_t)N * std::max(groups, C) * 16;
  *scratch = talloc(e, 1, 1, 1, (int)((sum_bytes + (size_t)N * C * 8 + 3) / 4), 1);
  *scale_out = nullptr; *shift_out = nullptr;
  if (e->dry) return 0;
  double* sums = (double*)scratch->p;
  float* scale = (float*)((unsigned char*)scratch->p + sum_bytes);
  float* shift = scale + (size_t)N * C;
  *scale_out = scale; *shift_out = shift;
  if (have_stats) {
    prof_begin(e, "gn_reduce", 0, ((double)rows0 * C0 + (double)rows1 * C1) * N * 8);
    SDM_LAUNCH(gn_partials_scale_shift_kernel, dim3(groups, N), dim3(GN_PSS_THREADS), 0, e->stream, st0, rows0, st1, rows1, C0, C1, gamma, beta, scale, shift,
               groups, (long)HW, eps);
    prof_end(e);
  } else {
    GnSrc s; s.in0 = in0; s.in1 = in1; s.C0 = C0; s.C1 = C1; s.in_f32 = in_f32; s.HW = HW;
    const GnGeometry g = gn_geometry(C, N, HW);
    SDM_CHECK_DEV(e, dev_memset(sums, 0, (size_t)N * groups * 16, e->stream));
    prof_begin(e, "gn_stats", 0, (double)N * HW * C * (in_f32 ? 4 : 2));
    SDM_LAUNCH(gn_stats_kernel, dim3(g.nb, N), dim3(g.threads), (size_t)2 * C * 4, e->stream, s, sums, groups, g.ppb);
    prof_end(e);
    SDM_LAUNCH(gn_finalize_kernel, dim3(sdm_cdiv(N * C, 256)), dim3(256), 0, e->stream, s, (const double*)sums, gamma, beta, scale, shift, N, C,
               groups, (long)HW * (C / groups), eps);
  }
  return 0;
}

static int op_groupnorm_raw(sdm_ctx* e, const void* in0, const void* in1, int C0, int C1, int in_f32, int N, int HW, int groups,
                            const float* gamma, const float* beta, float eps, int silu, void* out, int out_f32, const float* st0 = nullptr,
                            int rows0 = 0, const float* st1 = nullptr, int rows1 = 0, bool have_stats = false, int pt_W = 0) {
  const int C = C0 + C1;
  T scratch; float* scale; float* shift;
  // pt_W: width of the image whose P3 rows are written in patch token order (sdm_common.h), 0 = row-major
  if (pt_W && (out_f32 != kFmtP3 || HW % pt_W || !sdm_patch_tokens_ok(HW / pt_W, pt_W))) SDM_FAIL(e, SDM_ERR_INVALID, "groupnorm: patch token order needs P3 output and whole 8x8 patches");
  TRY(gn_scale_shift(e, in0, in1, C0, C1, in_f32, N, HW, groups, gamma, beta, eps, st0, rows0, st1, rows1, have_stats, &scratch, &scale, &shift));
  if (!e->dry) {
    GnSrc s; s.in0 = in0; s.in1 = in1; s.C0 = C0; s.C1 = C1; s.in_f32 = in_f32; s.HW = HW;
    const GnGeometry g = gn_geometry(C, N, HW);
    prof_begin(e, "gn_apply", 0, (double)N * HW * C * (in_f32 ? 4 : 2) + (double)N * HW * C * (double)fmt_bytes(out_f32));
    if (out_f32 == kFmtP3)
      SDM_LAUNCH(gn_apply_p3_kernel, dim3((unsigned)(((long)N * HW + 15) / 16)), dim3(256), 0, e->stream, s, (const float*)scale, (const float*)shift, (unsigned char*)out,
                 silu, (long)N * HW, pt_W);
    else
    SDM_LAUNCH(gn_apply_kernel, dim3(g.nb, N), dim3(g.threads), 0, e->stream, s, (const float*)scale, (const float*)shift, out, out_f32, silu, g.ppb);
    prof_end(e);
  }
  tfree(e, scratch);
  return 0;
}

static int op_gn(sdm_ctx* e, const NormL& n, const T& x, const T* x2, int silu, float eps, T* out, int out_fmt = -1, bool patch_tokens = false) {
  const int C = x.C + (x2 ? x2->C : 0);
  if (C != n.C) SDM_FAIL(e, SDM_ERR_INVALID, "groupnorm: C %d != %d", C, n.C);
  *out = talloc(e, x.N, x.H, x.W, C, out_fmt >= 0 ? out_fmt : e->act_f32);
  const bool hs = x.sbytes && (!x2 || x2->sbytes);     // statistics already produced by the conv epilogue(s)
  return op_groupnorm_raw(e, x.p, x2 ? x2->p : nullptr, x.C, x2 ? x2->C : 0, x.f32, x.N, x.H * x.W, e->cfg.groups, n.g, n.b, eps, silu,
                          out->p, out->f32, x.stats, x.srows, x2 ? x2->stats : nullptr, x2 ? x2->srows : 0, hs, patch_tokens ? x.W : 0);
}

static int op_ln(sdm_ctx* e, const NormL& n, const T& x, float eps, T* out, int out_fmt = -1) {
  if (x.C != n.C || x.C % 64 || x.C > 64 * SDM_LN_MAXV) SDM_FAIL(e, SDM_ERR_INVALID, "layernorm: unsupported C %d", x.C);
  *out = talloc(e, x.N, x.H, x.W, x.C, out_fmt >= 0 ? out_fmt : e->act_f32);
  if (e->dry) return 0;
  const long rows = x.rows();
  if (out->f32 == kFmtP3) {
    if (x.f32 != 1 || x.C > 128 * SDM_LNP_MAXI) SDM_FAIL(e, SDM_ERR_INVALID, "layernorm (P3): fp32 input, C <= %d expected", 128 * SDM_LNP_MAXI);
    prof_begin(e, "layernorm", 0, (double)rows * x.C * 7);
    SDM_LAUNCH(layernorm_p3_kernel, dim3((unsigned)((rows + 15) / 16)), dim3(256), 0, e->stream, (const float*)x.p, (const float*)n.g, (const float*)n.b,
               (unsigned char*)out->p, rows, x.C, eps);
    prof_end(e);
    return 0;
  }
  prof_begin(e, "layernorm", 0, (double)rows * x.C * ((x.f32 ? 4 : 2) + (out->f32 ? 4 : 2)));
  SDM_LAUNCH(layernorm_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, e->stream, (const void*)x.p, x.f32, (const float*)n.g,
             (const float*)n.b, out->p, out->f32, rows, x.C, eps);
  prof_end(e);
  return 0;
}

// q/k/v are views into fp16 row-major buffers; v is transposed into an arena scratch first
// Precise variant (d = 64): q / k / v point at the HIGH planes of split fp16 pairs, the low planes follow at element offsets
// q_lo / k_lo / v_lo (written by the producing GEMM with out_f32 == 2); `out` is fp16 or fp32 (out_f32).
// prec: 0 fp16 operands; 1 q / k / v as fp16 planes hi | lo; 2 q / k as fp16 plane + e5m2 pair plane (ConvParams::out_f32 == 3), v hi only
// has_bias / has_tiles: whether a key bias / a caller's tile list comes with the call.  Stated by the caller, never read off bias_l2 / tiles: those
// pointers exist only outside the dry pass, and the launch plan must be the same in both passes.
// shared_kv (d = 64, no residual terms of P.V): ONE key / value operand for every head - `k` is [b][key][64] (ldk = 64, head stride 0) and `v` is the READY
// V^T [b][64][rup(Lk, 64)] (zero filled behind Lk; ldv is not read): no V^T scratch, no transpose_v launch
// narrow36 (with shared_kv; set by cross_attention alone, for planes that cross_patch_planes_kernel wrote with ones_rows): columns 36..63 of q and k are zero and
// V^T rows 59 / 63 hold 1.0 - the launch plan may take the narrow form of a core (k_attn.h NARROW).  NOT implied by shared_kv: a caller's operand
// (sdm_op_attention_shared) may have live columns up to 63 and has no ones rows.
struct AttnPrec { int prec = 0; long q_lo = 0, k_lo = 0, v_lo = 0; int out_f32 = 0; int out_p3 = 0; bool has_bias = false, has_tiles = false; bool shared_kv = false; bool narrow36 = false; };      // out_p3 (with out_f32 = 1): `out` is a P3 tensor (k_gemm.h)

// Everything op_attention_raw decides about a launch, decided once: the sizing pass allocates from it, the launch pass launches from it.
enum AttnKernel { kAttnPP, kAttnPPBias, kAttnPPTiles, kAttnPPNarrow, kAttnPipe8, kAttnPipe4, kAttnPipe4Narrow, kAttnP3W8, kAttnP3W4, kAttnP1W8, kAttnP1W4, kAttnP2W8, kAttnP2W4,
                  kAttnF16W8, kAttnF16W4, kAttnD512, kAttnD512PP };
struct AttnPlan {
  AttnKernel kernel;              // row of kAttnKernels: launch counter (d = 64 launches are counted), block size, dynamic LDS
  const char* spec_counter;       // ping-pong kernel: the specialisation taken (tests); otherwise null
  const char* combine_counter;    // nsplit > 1: the split taken (tests); otherwise null
  int qrows;                      // query rows per block
  unsigned nblk;                  // grid.x: 1-D, XCD-aware mapping in the kernel
  int nsplit;                     // key split (k_attn.h AttnParams::nsplit) = grid.y; 1: unsplit
  bool walk_tiles, own_list;      // the kernel walks a list of active key tiles; the operator builds that list itself
  bool pv_split;                  // residual terms of P.V too: V^T_lo is needed as well
  int pp_flags;
  bool narrow;                    // the narrow form of the kernel (AttnPrec::narrow36 and a kernel that has one): counted as attn_d64_narrow
};
struct AttnKernelInfo { const char* counter; int threads; size_t smem; void (*launch)(const AttnKernelInfo&, const AttnPlan&, const AttnParams&, void*); };
template <auto K, int LDS_LIMIT = 160 * 1024>      // LDS_LIMIT: the dynamic-LDS limit the kernel is given (0: the default limit holds its LDS)
static void attn_launch_t(const AttnKernelInfo& ki, const AttnPlan& pl, const AttnParams& p, void* stream) {
  if constexpr (LDS_LIMIT > 0) SDM_SET_SMEM(K, LDS_LIMIT);
  SDM_LAUNCH(K, dim3(pl.nblk, (unsigned)pl.nsplit, 1), dim3(ki.threads), ki.smem, stream, p);
}
static const AttnKernelInfo kAttnKernels[] = {      // indexed by AttnKernel
  {"attn_d64_pp", 512, ATTN64PP_SMEM, attn_launch_t<attn_d64_pp_kernel<0, 0, 0>>},
  {"attn_d64_pp", 512, ATTN64PP_SMEM, attn_launch_t<attn_d64_pp_kernel<0, 1, 0>>},
  {"attn_d64_pp", 512, ATTN64PP_SMEM, attn_launch_t<attn_d64_pp_kernel<0, 1, 1>>},
  {"attn_d64_pp", 512, ATTN64PP_SMEM, attn_launch_t<attn_d64_pp_kernel<0, 0, 0, 0, 1, 1, 1>>},
  {"attn_d64_pipe<8>", 512, ATTN64PIPE_SMEM, attn_launch_t<attn_d64_pipe_kernel<8>>},
  {"attn_d64_pipe<4>", 256, ATTN64PIPE4_SMEM, attn_launch_t<attn_d64_pipe_kernel<4>>},
  {"attn_d64_pipe<4>", 256, ATTN64PIPE4_SMEM, attn_launch_t<attn_d64_pipe_kernel<4, 1>>},
  {"attn_d64<prec3,8>", 512, ATTN64P_SMEM, attn_launch_t<attn_d64_kernel<1, 3, 8>>},
  {"attn_d64<prec3,4>", 256, ATTN64P_SMEM, attn_launch_t<attn_d64_kernel<1, 3, 4>>},
  {"attn_d64<prec1,8>", 512, ATTN64P_SMEM, attn_launch_t<attn_d64_kernel<1, 1, 8>>},
  {"attn_d64<prec1,4>", 256, ATTN64P_SMEM, attn_launch_t<attn_d64_kernel<1, 1, 4>>},
  {"attn_d64<prec2,8>", 512, ATTN64P_SMEM, attn_launch_t<attn_d64_kernel<1, 2, 8>>},
  {"attn_d64<prec2,4>", 256, ATTN64P_SMEM, attn_launch_t<attn_d64_kernel<1, 2, 4>>},
  {"attn_d64<fp16,8>", 512, ATTN64P_SMEM, attn_launch_t<attn_d64_kernel<1, 0, 8>>},
  {"attn_d64<fp16,4>", 256, ATTN64_SMEM, attn_launch_t<attn_d64_kernel<1, 0, 4>, 0>},
  {"attn_d512", 512, ATTN512P_SMEM, attn_launch_t<attn_d512_kernel<0>, ATTN512P_SMEM>},
  {"attn_d512_pp", 512, ATTN512P_SMEM, attn_launch_t<attn_d512_pp_kernel<0>, ATTN512P_SMEM>},
};
// Pure: shapes, flags, the options and the CU count in, the plan out.
static AttnPlan attn_plan(int B, int heads, int Lq, int Lk, int D, int prec, int out_f32, bool has_bias, bool has_tiles, int cus, bool narrow36 = false) {
  AttnPlan pl;
  memset(&pl, 0, sizeof(pl));
  pl.nsplit = 1;
  bool nw8 = true, pp = false;      // (d = 512: one 8-wave kernel, 128 query rows per block)
  if (D != 64) {
    const int pp5 = opt("attn512_pp");
    pl.kernel = pp5 ? kAttnD512PP : kAttnD512; pl.qrows = 128;
    pl.pp_flags = pp5 == 1 ? 1 : 0;
  } else {
    // key tiles whose bias underflows the softmax are skipped (exact, AttnParams::tiles); the engine passes one list per U-Net
    // level, the stand-alone operator entry builds it here.  The option attn_dense = 1 walks every tile (A/B hook).
    pl.walk_tiles = has_bias && opt("attn_dense") == 0;
    pl.own_list = pl.walk_tiles && !has_tiles;
    // split-precision variant: Q.K^T on split operands, P.V on plain fp16 (k_attn.h, PREC = 2) unless the option attn_pv_split asks for
    // the residual terms of P.V too (PREC = 1)
    pl.pv_split = prec == 1 && opt("attn_pv_split") != 0;
    // 8-wave blocks (256 queries share every K / V^T tile: half the L2 / Infinity-Cache traffic and LDS staging per MFMA) only
    // where they measured faster: the split-precision variant with >= 4 such blocks per CU (B=4 h=5 L=16384: 4.01 vs 4.25 ms;
    // h=10 Lq=4096: 2.39 vs 2.24 ms, i.e. slower; the fp16 variant is neutral to -10 %) - profiles/r02_ablate_attn_nw8.txt
    const int force_nw = opt("attn_nw");                          // A/B / test option: 4 or 8
    const long blocks256 = (long)B * heads * sdm_cdiv(Lq, 256);
    // ping-pong kernel: always 256-row blocks, one per CU; launches of fewer than 128 such blocks (the 16^2 level: 80) keep the 4-wave pipelines, whose 128-row
    // blocks spread over twice as many CUs (measured 0.63 vs 0.79 ms at B = 4, profiles/r06_attn_pp_lab.txt)
    pp = prec == 2 && out_f32 && opt("attn_pp") != 0 && !force_nw && Lk % 64 == 0 &&      // (LDS-DMA tiles: no masked tail rows)
         blocks256 >= opt("attn_pp_min_blocks");
    nw8 = pp || (force_nw ? (force_nw == 8) : (prec && blocks256 >= 1024));
    pl.qrows = nw8 ? 256 : 128;
    if (prec == 2) {
      // 8-wave blocks with fp32 output (the engine's level-0 attentions): the two-tile software pipeline of the kernel (k_attn.h,
      // attn_d64_pipe_kernel: same arithmetic, bit-identical results, -9 % kernel time); option attn_pipe = 0 selects the plain form.
      const bool pipe = out_f32 && opt(nw8 ? "attn_pipe" : "attn_pipe4") != 0;
      if (pp) pl.kernel = pl.walk_tiles ? kAttnPPTiles : (has_bias ? kAttnPPBias : kAttnPP);
      else if (pipe) pl.kernel = nw8 ? kAttnPipe8 : kAttnPipe4;
      else pl.kernel = nw8 ? kAttnP3W8 : kAttnP3W4;
    } else if (prec) {
      pl.kernel = pl.pv_split ? (nw8 ? kAttnP1W8 : kAttnP1W4) : (nw8 ? kAttnP2W8 : kAttnP2W4);
    } else {
      pl.kernel = nw8 ? kAttnF16W8 : kAttnF16W4;
    }
    // narrow form (AttnPrec::narrow36): the ping-pong kernel without bias and the 4-wave pipeline have one, at whole 64-key tiles; every other launch (the
    // 8-wave pipeline, the plain kernels, a ragged last tile) runs the full program on the same operand - the ones rows then only fill dead output columns
    if (narrow36 && !has_bias && Lk % 64 == 0) {
      if (pl.kernel == kAttnPP) { pl.kernel = kAttnPPNarrow; pl.narrow = true; }
      else if (pl.kernel == kAttnPipe4) { pl.kernel = kAttnPipe4Narrow; pl.narrow = true; }
    }
    if (pp) {
      pl.spec_counter = pl.walk_tiles ? "attn_pp<0,1,1>" : (has_bias ? "attn_pp<0,1,0>" : "attn_pp<0,0,0>");
      pl.pp_flags = opt("attn_pp") == 1 ? 1 : (opt("attn_pp") == 3 ? 2 : 0);
    }
  }
  pl.nblk = (unsigned)(B * heads * 8 * sdm_cdiv(sdm_cdiv(Lq, pl.qrows), 8));      // B * heads * 8 units: always a multiple of 8
  // Key split (split-precision d = 64 with fp32 output only).  A launch whose blocks fill the chip's block slots 1.25 times
  // takes as long as one that fills them twice; walking half (a quarter) of the keys per block and combining the partial sums afterwards turns
  // that into 2.5 (5) rounds of half (quarter) length.  Chosen by block count alone - the same for the dense and the tile-list walk, whose ranges are key
  // ranges - and only for long walks (>= 32 tiles per part).  One image at 1024^2: 640 four-wave blocks on 512 slots at the first U-Net level.
  if (D == 64 && prec && out_f32 && !pl.pv_split) {
    const long blocks = pl.nblk, slots = (long)cus * (nw8 ? 1 : 2);
    const int o = opt("attn_ksplit"), ntiles64 = sdm_cdiv(Lk, 64);
    if (o >= 2) pl.nsplit = (o == 2 || o == 4 || (o == 3 && pp)) ? o : 1;
    else if (o == 0) {
      auto rounds = [&](int s) { return (double)((blocks * s + slots - 1) / slots) / s; };
      for (int s = 2; s <= 4; ++s)      // (3: 80 one-per-CU blocks - the 16^2 level's cross-attentions - become 240 of a third of the length)
        if ((s != 3 || pp) && ntiles64 / s >= 32 && rounds(s) < 0.85 * rounds(pl.nsplit)) pl.nsplit = s;
    }
    if (pl.nsplit > 1) pl.combine_counter = pl.nsplit == 2 ? "attn_combine/n=2" : (pl.nsplit == 3 ? "attn_combine/n=3" : "attn_combine/n=4");
  }
  return pl;
}

static int op_attention_raw(sdm_ctx* e, const half_t* q, int ldq, const half_t* k, int ldk, const half_t* v, int ldv, const float* bias_l2,
                            int B, int heads, int Lq, int Lk, int D, void* out, int ldo, bool q_prescaled = false, const int* tiles = nullptr,
                            AttnPrec ap = AttnPrec()) {
  if (!(D == 64 || (D == 512 && heads == 1))) SDM_FAIL(e, SDM_ERR_INVALID, "attention: unsupported head dim %d x %d heads", D, heads);
  if ((ldq | ldk | ldv | ldo) % 8) SDM_FAIL(e, SDM_ERR_INVALID, "attention: row strides must be multiples of 8");
  if (ap.prec && D != 64) SDM_FAIL(e, SDM_ERR_INVALID, "attention: the split-precision variant exists for head dim 64 only");
  // the fp8-pair form cannot rescale Q inside the kernel (its pair plane is produced pre-scaled, as the engine always does)
  if (ap.prec == 2 && !q_prescaled) SDM_FAIL(e, SDM_ERR_INVALID, "attention: the fp8-residual form takes pre-scaled queries");
  if (!e->dry && (ap.has_bias != (bias_l2 != nullptr) || ap.has_tiles != (tiles != nullptr)))
    SDM_FAIL(e, SDM_ERR_STATE, "attention: bias / tile list do not match what the sizing pass was told");
  if (ap.narrow36 && !ap.shared_kv) SDM_FAIL(e, SDM_ERR_INVALID, "attention: the narrow form exists for the shared key / value operand only");
  const AttnPlan pl = attn_plan(B, heads, Lq, Lk, D, ap.prec, ap.out_f32, ap.has_bias, ap.has_tiles, device_cus(), ap.narrow36);
  const AttnKernelInfo& ki = kAttnKernels[pl.kernel];
  const int nsplit = pl.nsplit;
  const int ldvt = rup(Lk, 64);
  if (ap.shared_kv && (D != 64 || pl.pv_split || ldk != 64)) SDM_FAIL(e, SDM_ERR_INVALID, "attention: a shared key / value operand is [key][64] at head dim 64, without the residual terms of P.V");
  T vt;
  if (!ap.shared_kv) vt = talloc(e, (ap.prec ? 2 : 1) * B, heads, D, ldvt, 0);      // precise: V^T_hi planes of all images, then V^T_lo
  const int ntiles64 = sdm_cdiv(Lk, 64);
  T tl_own, part_o, part_ml;
  if (pl.own_list) tl_own = talloc(e, B, 1, 1, ntiles64 + 1, 1);
  if (nsplit > 1) {
    part_o = talloc(e, nsplit * B, Lq, 1, ldo, 1);
    part_ml = talloc(e, nsplit * B, heads, Lq, 2, 1);
  }
  if (!e->dry) {
    if (pl.own_list) {
      SDM_LAUNCH(attn_active_tiles_kernel, dim3(B), dim3(256), 0, e->stream, bias_l2, Lk, ntiles64, (int*)tl_own.p, ntiles64 + 1, SDM_ATTN_SKIP_MARGIN);
      tiles = (const int*)tl_own.p;
    }
    if (!pl.walk_tiles) tiles = nullptr;
    const long vt_hs = ap.shared_kv ? 0 : (long)D * ldvt, vt_bs = ap.shared_kv ? (long)D * ldvt : (long)heads * vt_hs;
    if (!ap.shared_kv) {
      prof_begin(e, "transpose_v", 0, (double)B * Lk * heads * D * 4);
      count_kernel("transpose_v");
      SDM_LAUNCH(transpose_v_kernel, dim3(ldvt / 64, heads * (D / 64), B), dim3(256), 0, e->stream, v, (long)Lk * ldv, ldv, (half_t*)vt.p, vt_bs,
                 vt_hs, ldvt, Lk, D);
      if (pl.pv_split)
        SDM_LAUNCH(transpose_v_kernel, dim3(ldvt / 64, heads * (D / 64), B), dim3(256), 0, e->stream, v + ap.v_lo, (long)Lk * ldv, ldv,
                   (half_t*)vt.p + (size_t)B * vt_bs, vt_bs, vt_hs, ldvt, Lk, D);
      prof_end(e);
    }
    AttnParams p;
    memset(&p, 0, sizeof(p));
    p.q = q; p.q_bs = (long)Lq * ldq; p.ldq = ldq;
    p.k = k; p.k_bs = (long)Lk * ldk; p.ldk = ldk; p.k_hs = ap.shared_kv ? 0 : 64;
    p.vt = ap.shared_kv ? v : (const half_t*)vt.p; p.vt_bs = vt_bs; p.vt_hs = vt_hs; p.ldvt = ldvt;
    p.bias = bias_l2; p.bias_bs = Lk;
    p.tiles = tiles; p.tiles_bs = ntiles64 + 1;
    p.o = (half_t*)out; p.o_bs = (long)Lq * ldo; p.ldo = ldo; p.o_f32 = ap.out_f32;
    if (ap.out_p3) {
      if (!ap.out_f32 || Lq % 32 || ldo % 32 || D != 64) SDM_FAIL(e, SDM_ERR_INVALID, "attention: plane output needs d = 64, Lq %% 32 == 0 and C %% 32 == 0");
      p.o_p3 = 1; p.o_xl_off = (long)(p3_rows_pad((size_t)B * Lq) * ldo * 2);
    }
    p.q_lo = ap.q_lo; p.k_lo = ap.k_lo; p.vt_lo = (long)B * vt_bs;
    p.Lq = Lq; p.Lk = Lk;
    p.scale_log2e = q_prescaled ? 1.0f : (1.0f / sqrtf((float)D)) * SDM_LOG2E;      // engine: folded into the to_q weights (d = 64 only)
    if (nsplit > 1) { p.nsplit = nsplit; p.o = (half_t*)part_o.p; p.part_stride = (long)B * p.o_bs; p.part_ml = (float*)part_ml.p; }
    p.batch = B; p.heads = heads; p.nq_blocks = sdm_cdiv(Lq, pl.qrows); p.q_chunks = 8;
    p.pp_flags = pl.pp_flags;
    double flops = 4.0 * B * heads * (double)Lq * Lk * D;
    const double bytes = 2.0 * B * heads * D * (2.0 * Lq + 2.0 * Lk);
    std::string adesc = "B=" + std::to_string(B) + " h=" + std::to_string(heads) + " Lq=" + std::to_string(Lq) + " Lk=" + std::to_string(Lk);
    if (e->prof_on && tiles) {      // profiling only: report EXECUTED flops - needs the tile counts on the host
      std::vector<int> hl((size_t)B * (ntiles64 + 1));
      (void)dev_sync(e->stream);
      (void)dev_memcpy_d2h(hl.data(), tiles, hl.size() * sizeof(int), e->stream);
      (void)dev_sync(e->stream);
      long act = 0;
      for (int bi = 0; bi < B; ++bi) act += hl[(size_t)bi * (ntiles64 + 1)];
      const double frac = (double)act / ((double)B * ntiles64);
      flops *= frac;
      char fb[48];
      snprintf(fb, sizeof(fb), " active_key_tiles=%.3f", frac);
      adesc += fb;
    }
    if (D == 64) {
      prof_begin(e, "attn_d64", flops, bytes, adesc);
      count_kernel(ki.counter);
      if (pl.spec_counter) count_kernel(pl.spec_counter);
      if (pl.narrow) count_kernel("attn_d64_narrow");
      ki.launch(ki, pl, p, e->stream);
      if (nsplit > 1) {
        count_kernel("attn_combine");
        count_kernel(pl.combine_counter);
        if (ap.out_p3) count_kernel("attn_combine_p3");
        const long nthr = (long)B * Lq * heads * 16;
        if (ap.out_p3)
          SDM_LAUNCH(attn_combine_p3_kernel, dim3((unsigned)((nthr / 2 + 255) / 256)), dim3(256), 0, e->stream, (const float*)part_o.p, (const float*)part_ml.p,
                     (unsigned char*)out, (long)(p3_rows_pad((size_t)B * Lq) * ldo * 2), nsplit, (long)B * (long)Lq * ldo, B, heads, Lq, (long)Lq * ldo, ldo);
        else
        SDM_LAUNCH(attn_combine_kernel, dim3((unsigned)((nthr + 255) / 256)), dim3(256), 0, e->stream, (const float*)part_o.p, (const float*)part_ml.p, (float*)out,
                   nsplit, (long)B * (long)Lq * ldo, B, heads, Lq, (long)Lq * ldo, ldo);
      }
      prof_end(e);
    } else {
      prof_begin(e, "attn_d512", flops, bytes);
      if (pl.kernel == kAttnD512PP) count_kernel(ki.counter);
      ki.launch(ki, pl, p, e->stream);
      prof_end(e);
    }
  }
  if (nsplit > 1) { tfree(e, part_ml); tfree(e, part_o); }
  if (pl.own_list) tfree(e, tl_own);
  if (!ap.shared_kv) tfree(e, vt);
  return 0;
}


// ------------------------------------------------------------------------------------------------
// blocks
// ------------------------------------------------------------------------------------------------
static int conv_simple(sdm_ctx* e, int layer, const T& in, T* out, int Cout_store, int out_f32, int stride = 1, int pad_mode = 0, int up = 0,
                       const T* res = nullptr, float scale = 1.0f, bool want_stats = false, int lo_cols = -1) {
  const ConvL& L = e->convs[layer];
  int Ho = in.H << up, Wo = in.W << up;
  if (stride == 2) { Ho /= 2; Wo /= 2; }
  *out = talloc(e, in.N, Ho, Wo, Cout_store, out_f32);
  if (want_stats) TRY(tstats(e, *out));
  ConvArgs a; a.in0 = &in; a.out = out; a.stride = stride; a.pad_mode = pad_mode; a.up = up; a.res = res; a.out_scale = scale; a.lo_cols = lo_cols;
  return op_conv(e, L, a);
}

// GroupNorm(32)(+SiLU) followed by a 3x3 stride-1 conv.  When the conv runs on the 256x128 tile the normalisation is applied
// inside the conv's operand staging (no normalised copy of the activation is ever written); otherwise the stand-alone apply
// kernel produces the fp16 operand first.  `a` carries everything except the inputs.
static int gn_conv(sdm_ctx* e, const NormL& n, const ConvL& L, const T& x, const T* x2, int silu, float eps, ConvArgs a) {
  const int C = x.C + (x2 ? x2->C : 0);
  if (C != n.C) SDM_FAIL(e, SDM_ERR_INVALID, "groupnorm: C %d != %d", C, n.C);
  // the tile op_conv would pick: the 256-pixel tiles (cfg 0 / 4 / 5) carry the fused-GroupNorm variant
  int cfg = -1;
  if (!opt("no_gn_fuse") && L.ntaps == 9 && a.stride == 1 && C <= 1024 && C == L.Cin_pad) {
    ConvParams p;
    memset(&p, 0, sizeof(p));
    conv_shape_params(p, L, x, x2, *a.out, a.stride);
    cfg = conv_pick_cfg(L.ntaps, a.stride, p);
  }
  if (cfg == 0 || cfg == 4 || cfg == 5) {
    const bool hs = x.sbytes && (!x2 || x2->sbytes);
    T scratch; float* scale; float* shift;
    TRY(gn_scale_shift(e, x.p, x2 ? x2->p : nullptr, x.C, x2 ? x2->C : 0, x.f32, x.N, x.H * x.W, e->cfg.groups, n.g, n.b, eps, x.stats, x.srows,
                       x2 ? x2->stats : nullptr, x2 ? x2->srows : 0, hs, &scratch, &scale, &shift));
    a.in0 = &x; a.in1 = x2;
    a.gn_scale = e->dry ? (const float*)16 : scale; a.gn_shift = shift; a.gn_silu = silu;
    a.force_cfg = cfg;
    int rc = op_conv(e, L, a);
    tfree(e, scratch);
    return rc;
  }
  T h;
  TRY(op_gn(e, n, x, x2, silu, eps, &h));
  a.in0 = &h; a.in1 = nullptr;
  int rc = op_conv(e, L, a);
  tfree(e, h);
  return rc;
}

// ResnetBlock2D (Appendix A.3).  x (+ x2: channel concat) -> new stream tensor; frees nothing.
static int resblock(sdm_ctx* e, const ResB& r, const T& x, const T* x2, float eps, T* out) {
  const int sf = e->cfg.stream_f32;
  T h1 = talloc(e, x.N, x.H, x.W, r.cout, e->act_f32);
  TRY(tstats(e, h1));
  {
    ConvArgs a; a.out = &h1;
    if (r.temb >= 0) { a.bias_override = e->tembs[r.temb].table; a.bias_sel = e->d_bias_sel; }
    TRY(gn_conv(e, e->norms[r.norm1], e->convs[r.conv1], x, x2, 1, eps, a));
  }
  T xs; const T* resid = &x;
  if (r.sc >= 0) {
    xs = talloc(e, x.N, x.H, x.W, r.cout, sf);
    ConvArgs a; a.in0 = &x; a.in1 = x2; a.out = &xs;
    TRY(op_conv(e, e->convs[r.sc], a));
    resid = &xs;
  } else if (x2) {
    SDM_FAIL(e, SDM_ERR_INVALID, "resblock: concat input without shortcut");
  }
  *out = talloc(e, x.N, x.H, x.W, r.cout, sf);
  TRY(tstats(e, *out));
  {
    ConvArgs a; a.out = out; a.res = resid;
    TRY(gn_conv(e, e->norms[r.norm2], e->convs[r.conv2], h1, nullptr, 1, eps, a));
  }
  tfree(e, h1);
  if (r.sc >= 0) tfree(e, xs);
  return 0;
}

// ---- plane-fed GEMM path (k_gemm.h).  `in` is a P3 tensor (T::f32 == kFmtP3); the output format picks the epilogue: fp32 (+residual, +statistics),
//      P3 (GEGLU layers, or linear + residual), or the q | k | v operand planes of the attention cores (format 3) ----
static bool p3_ok(sdm_ctx* e, const ConvL& L) { return L.w3 != nullptr && e->act_f32 && opt("gemm_p3") != 0; }
// patch_tokens: `in` holds the rows of its images in patch token order (sdm_common.h), `out` and `res` are pixel-order NHWC (epilogues 0 / 4 only)
static int op_gemm_p3(sdm_ctx* e, const ConvL& L, const T& in, T* out, const T* res, int lo_cols, bool patch_tokens = false) {
  if (in.f32 != kFmtP3 || in.C != L.Cin_pad) SDM_FAIL(e, SDM_ERR_INVALID, "gemm %s: needs a P3 operand of %d channels", L.name.c_str(), L.Cin_pad);
  if (!L.w3) SDM_FAIL(e, SDM_ERR_STATE, "gemm %s: no W3 weight copy", L.name.c_str());
  if (res && res->f32 != 1) SDM_FAIL(e, SDM_ERR_INVALID, "gemm %s: fp32 residual expected", L.name.c_str());
  const int nout = L.geglu ? L.Cout_pad / 2 : L.Cout_pad;
  if (out->C % 32 || std::min(nout, out->C) % 32) SDM_FAIL(e, SDM_ERR_INVALID, "gemm %s: output channels %d", L.name.c_str(), out->C);
  int epi;
  if (L.geglu) { if (out->f32 != kFmtP3) SDM_FAIL(e, SDM_ERR_INVALID, "gemm %s: GEGLU writes P3", L.name.c_str()); epi = 1; }
  else if (out->f32 == 1) epi = out->want_stats ? 4 : 0;
  else if (out->f32 == 3) epi = 2;
  else if (out->f32 == 0) { epi = 2; lo_cols = 0; }          // plain fp16 rows = the high plane alone (q | k | v of the d = 512 attention)
  else if (out->f32 == kFmtP3) epi = 3;
  else SDM_FAIL(e, SDM_ERR_INVALID, "gemm %s: unsupported output format %d", L.name.c_str(), out->f32);
  GemmP3Params p;
  memset(&p, 0, sizeof(p));
  p.M = in.rows(); p.K = L.Cin_pad;
  p.a_hi = (const half_t*)in.p; p.a_xl = (const unsigned char*)in.p + p3_rows_pad((size_t)p.M) * p.K * 2;
  p.w = L.w3; p.N = L.Cout_pad; p.bias = L.b;
  p.out = out->p; p.ldo = out->C; p.n_valid = std::min(nout, out->C);
  p.out_lo_off = (epi == 2) ? (size_t)out->rows() * out->C : p3_rows_pad((size_t)out->rows()) * out->C * 2;
  p.lo_cols = lo_cols >= 0 ? lo_cols : (1 << 30);
  if (res) { p.res = (const float*)res->p; p.ldr = res->C; }
  p.sa = 127 - 11; p.sb = 127 - L.f8_exp;
  if (epi == 4) {
    if ((in.H * in.W) % 32) SDM_FAIL(e, SDM_ERR_INVALID, "gemm %s: fused statistics need images of a multiple of 32 rows (blocked operand planes)", L.name.c_str());
    p.rows_per_img = in.H * in.W;
    const int bm = gemm_p3_pick_bm(p.M, p.N, p.rows_per_img);
    out->srows = sdm_cdiv(p.rows_per_img, bm) * 2;
    T sb = talloc(e, 1, 1, 1, (int)((size_t)in.N * out->srows * out->C * 2), 1);
    out->soff = sb.off; out->sbytes = sb.bytes; out->stats = (float*)sb.p;
    p.stats = out->stats;
  }
  if (patch_tokens) {
    if ((epi != 0 && epi != 4) || !sdm_patch_tokens_ok(in.H, in.W)) SDM_FAIL(e, SDM_ERR_INVALID, "gemm %s: patch token order needs an fp32 output and whole 8x8 patches", L.name.c_str());
    p.rows_per_img = in.H * in.W; p.pt_W = in.W;
    // a tile's descriptors span the pixel rows of the patch rows it touches (k_gemm.h): at most ceil(4 / (W / 8)) + 1 of them with the 256-row tile
    const double span = (double)(sdm_cdiv(4, in.W / 8) + 1) * 8.0 * in.W * std::max(p.ldo, p.ldr) * 4.0;
    if (span >= (double)SDM_BUF_INVALID) SDM_FAIL(e, SDM_ERR_INVALID, "gemm %s: a tile's pixel rows exceed the buffer descriptor range", L.name.c_str());
  }
  if (e->dry) return 0;
  if (epi == 4) TRY(stats_poison(e, *out));
  const double flops = 2.0 * (double)p.M * L.O * L.I;
  const double bytes = (double)p.M * p.K * 3 + (double)p.M * p.n_valid * (double)fmt_bytes(out->f32) + (double)p.K * p.N * 4 + (res ? (double)p.M * p.n_valid * 4 : 0.0);
  if (e->prof_on) {
    char d[256];
    snprintf(d, sizeof(d), "%s N=%d Hout=%d Wout=%d Cin=%d Cout=%d p3 epi=%d bm=%d%s", L.name.c_str(), in.N, in.H, in.W, L.Cin_pad, L.O, epi, gemm_p3_pick_bm(p.M, p.N, p.rows_per_img),
             patch_tokens ? " patch_tokens" : "");
    prof_begin(e, "gemm_mfma", flops, bytes, d);
  } else {
    prof_begin(e, "conv", flops, bytes);
  }
  count_kernel("gemm_p3");
  launch_gemm_p3(p, epi, e->stream);
#ifndef SDM_EMU
  { const hipError_t le = hipGetLastError(); if (le != hipSuccess) SDM_FAIL(e, SDM_ERR_HIP, "gemm %s: launch failed: %s", L.name.c_str(), hipGetErrorString(le)); }
#endif
  prof_end(e);
  return 0;
}

// fp32 [rows][C] -> P3 (operands whose producer does not emit planes itself)
static int op_to_p3(sdm_ctx* e, const T& x, T* out) {
  if (x.f32 != 1 || x.C % 32) SDM_FAIL(e, SDM_ERR_INVALID, "to_p3: fp32 input with C %% 32 == 0 expected (C = %d)", x.C);
  *out = talloc(e, x.N, x.H, x.W, x.C, kFmtP3);
  if (e->dry) return 0;
  const long units = ((x.rows() + 31) / 32) * (x.C / 32);      // one wave per 32 rows x 32 channels
  prof_begin(e, "to_p3", 0, (double)x.rows() * x.C * 7);
  SDM_LAUNCH(to_p3_kernel, dim3((unsigned)std::min<long>((units + 3) / 4, 1 << 20)), dim3(256), 0, e->stream, (const float*)x.p, (unsigned char*)out->p, x.rows(), x.C);
  prof_end(e);
  return 0;
}

static int linear(sdm_ctx* e, int layer, const T& in, T* out, int Cout, int out_f32, const T* res = nullptr, bool want_stats = false, int lo_cols = -1,
                  bool patch_tokens = false) {
  *out = talloc(e, in.N, in.H, in.W, Cout, out_f32);
  if (want_stats) TRY(tstats(e, *out));
  if (in.f32 == kFmtP3) return op_gemm_p3(e, e->convs[layer], in, out, res, lo_cols, patch_tokens);
  if (patch_tokens) SDM_FAIL(e, SDM_ERR_STATE, "linear %s: patch token order without the plane-fed GEMM", e->convs[layer].name.c_str());
  ConvArgs a; a.in0 = &in; a.out = out; a.res = res; a.lo_cols = lo_cols;
  return op_conv(e, e->convs[layer], a);
}

// VAE mid-block Attention (Appendix A.5): GN -> q|k|v (+bias) -> softmax(qk^T/sqrt(C)) v -> to_out -> + x
static int vae_attention(sdm_ctx* e, const VaeAttnB& a, const T& x, T* out) {
  T hn, qkv, ao;
  // the single-head d=512 core always takes fp16 operands; a 64-channel VAE (test architectures) runs on the d=64 kernels and
  // follows the U-Net attention-core precision bit
  const int pa = ((e->cfg.precise_mask & SDM_PRECISE_UNET_ATTN) && a.C == 64) ? 1 : 0;
  // plane format of q | k | v: fp16 hi | lo (the logit scale is applied to Q inside the kernel here - it is not folded into these
  // weights - which the fp8 pair planes do not allow); V needs no low-part plane unless the fully split P.V form is requested
  const int pf = pa ? 2 : 0;
  const bool need_vlo = pf == 2 && opt("attn_pv_split") != 0;
  const int L = x.H * x.W;
  // plane-fed GEMMs (k_gemm.h) around the fp16-operand core: GroupNorm writes the q | k | v projection's operand planes, the projection plain fp16 rows,
  // the core fp32 rows that one pass converts to the planes of to_out - which adds the residual and emits the statistics of the next ResBlock's GroupNorm
  const bool p3 = pf == 0 && e->cfg.stream_f32 == 1 && L % 32 == 0 && a.C % 32 == 0 && p3_ok(e, e->convs[a.qkv]) && p3_ok(e, e->convs[a.out]);
  TRY(op_gn(e, e->norms[a.gn], x, nullptr, 0, e->cfg.vae_eps, &hn, p3 ? kFmtP3 : -1));
  TRY(linear(e, a.qkv, hn, &qkv, 3 * a.C, pf, nullptr, false, need_vlo ? -1 : 2 * a.C));
  tfree(e, hn);
  ao = talloc(e, x.N, x.H, x.W, a.C, e->act_f32);
  const half_t* q = (const half_t*)qkv.p;
  AttnPrec ap; ap.out_f32 = ao.f32; ap.prec = pa ? pf - 1 : 0;
  ap.q_lo = ap.k_lo = ap.v_lo = (long)qkv.rows() * qkv.C;
  TRY(op_attention_raw(e, q, 3 * a.C, q ? q + a.C : nullptr, 3 * a.C, q ? q + 2 * a.C : nullptr, 3 * a.C, nullptr, x.N, 1, L, L, a.C,
                       ao.p, a.C, false, nullptr, ap));
  tfree(e, qkv);
  if (p3) { T ap3; TRY(op_to_p3(e, ao, &ap3)); tfree(e, ao); ao = ap3; }      // (the d = 512 core keeps its fp32 epilogue: k_attn.h AttnParams::o_p3)
  TRY(linear(e, a.out, ao, out, a.C, e->cfg.stream_f32, &x, true));
  tfree(e, ao);
  return 0;
}

// Transformer2DModel + BasicTransformerBlock (Appendix A.7); masked: the self-attention takes the level's key bias [N][L] (log2 domain) and its list of
// active key tiles (bias / tiles: null in the sizing pass, which has no memory)
// plane format of the U-Net attentions' q | k | v: 0 fp16 rows, 2 fp16 hi | lo planes, 3 fp16 hi + e5m2 pair plane (the default precision)
static int unet_attn_plane_fmt(const sdm_ctx* e) { return (e->cfg.precise_mask & SDM_PRECISE_UNET_ATTN) ? (attn_f8_enabled() ? 3 : 2) : 0; }

// The key / value operand that every cross-attention of a forward shares (fold_cross_kv, cross_patch_planes_kernel): built once in front of the first
// transformer block, freed behind the last.  k: [2][B][Lk][64] halves - the fp16 plane of all images, then their pair plane; vt: [B][64][ldvt].
// The rule (`on`): option cross_shared != 0, the fp8-pair plane format (unet_attn_plane_fmt == 3: the default precision) and an fp32 U-Net input.  Every
// other precision mode - the fp16 fast mode and the fp16 hi | lo planes of attn_f8 = 0 - keeps each block's own kv_folded conv + transpose.
// narrow (option cross_narrow != 0): V^T rows 59 and 63 hold 1.0 and the cores may run their narrow form (AttnPrec::narrow36).  Columns 59 and 63 of every
// head of the CORE OUTPUT then hold 1.0 (the denominator divided by itself) instead of 0, like 36..58 / 60..62 dead columns: they meet all-zero rows of out_shared, in
// its fp16 part and in its fp8 residual part alike (fold_cross_shared packs 36 live rows per head), so nothing behind out_shared sees them.
struct CrossPlanes { bool on = false, narrow = false; T k, vt; };
static int cross_planes_build(sdm_ctx* e, const T& uin, CrossPlanes* cp) {
  cp->on = opt("cross_shared") != 0 && unet_attn_plane_fmt(e) == 3 && uin.f32 == 1 && uin.C == 16;
  if (!cp->on) return 0;
  cp->narrow = opt("cross_narrow") != 0;
  const int B = uin.N, Lk = uin.H * uin.W, ldvt = rup(Lk, 64);
  cp->k = talloc(e, 2 * B, 1, Lk, 64, 0);
  cp->vt = talloc(e, B, 1, 64, ldvt, 0);
  if (e->dry) return 0;
  prof_begin(e, "cross_patch_planes", 0, (double)B * Lk * (16.0 + 64 * 6));
  count_kernel("cross_patch_planes");
  const long nthr = std::max((long)B * Lk * 8, (long)B * 64 * (ldvt / 8));
  SDM_LAUNCH(cross_patch_planes_kernel, dim3((unsigned)((nthr + 255) / 256), 2, 1), dim3(256), 0, e->stream, (const float*)uin.p, B, uin.H, uin.W,
             (half_t*)cp->k.p, (half_t*)cp->k.p + (size_t)B * Lk * 64, (half_t*)cp->vt.p, ldvt, cp->narrow ? 1 : 0);
  prof_end(e);
  return 0;
}
static void cross_planes_free(sdm_ctx* e, CrossPlanes* cp) {
  if (!cp->on) return;
  tfree(e, cp->vt); tfree(e, cp->k);
}

// plane-fed GEMMs (k_gemm.h) for every Linear of a transformer block, or for none
static bool transformer_p3(sdm_ctx* e, const TfB& t, int pf) {
  bool p3 = e->cfg.stream_f32 == 1 && pf == 3 && t.C % 32 == 0;
  for (int l : {t.proj_in, t.qkv1, t.o1, t.q2, t.o2, t.q2s, t.o2s, t.ff1, t.ff2, t.proj_out}) p3 = p3 && p3_ok(e, e->convs[l]);
  return p3;
}

// The cross-attention of a transformer block, from the normalised hidden state `n` (the block's operand format) to to_out + residual `res` -> *out (freed by the
// caller; `n` is freed here).  cp.on: Q~ = q_shared(n) attends to the shared operand, out_shared maps the 36 live columns per head back; otherwise
// to_q, the block's own kv_folded conv of the latent (+ transpose_v inside the operator), to_out.0.
static int cross_attention(sdm_ctx* e, const TfB& t, T& n, const T& uin, const CrossPlanes& cp, int pf, bool p3, bool p3a, const T* res, T* out) {
  const int C = t.C, N = n.N, H = n.H, W = n.W, L = H * W, L0 = uin.H * uin.W, sf = e->cfg.stream_f32;
  const int pa = pf ? 1 : 0;
  const bool need_vlo = pf == 2 && opt("attn_pv_split") != 0;
  T q2, kv, ao;
  TRY(linear(e, cp.on ? t.q2s : t.q2, n, &q2, C, pf));
  tfree(e, n);
  if (!cp.on) TRY(conv_simple(e, t.kv2, uin, &kv, 2 * C, pf, 1, 0, 0, nullptr, 1.0f, false, need_vlo ? -1 : C));      // folded aux_conv_in + to_k|to_v: tokens = latent pixels, row-major
  ao = talloc(e, N, H, W, C, p3a ? kFmtP3 : e->act_f32);
  {
    AttnPrec ap; ap.prec = pa ? pf - 1 : 0; ap.out_f32 = p3a ? 1 : ao.f32; ap.out_p3 = p3a ? 1 : 0;
    ap.q_lo = (long)q2.rows() * q2.C;
    if (cp.on) {
      const half_t* kk = (const half_t*)cp.k.p;
      ap.shared_kv = true; ap.narrow36 = cp.narrow; ap.k_lo = (long)N * L0 * 64;
      TRY(op_attention_raw(e, (const half_t*)q2.p, C, kk, 64, (const half_t*)cp.vt.p, 64, nullptr, N, t.heads, L, L0, 64, ao.p, C, true, nullptr, ap));
    } else {
      const half_t* kk = (const half_t*)kv.p;
      ap.k_lo = ap.v_lo = (long)kv.rows() * kv.C;
      TRY(op_attention_raw(e, (const half_t*)q2.p, C, kk, 2 * C, kk ? kk + C : nullptr, 2 * C, nullptr, N, t.heads, L, L0, 64, ao.p, C, true, nullptr, ap));
    }
  }
  tfree(e, q2);
  if (!cp.on) tfree(e, kv);
  if (p3 && !p3a) {      // the attention output as the next GEMM's operand
    T ap3;
    TRY(op_to_p3(e, ao, &ap3));
    tfree(e, ao);
    ao = ap3;
  }
  TRY(linear(e, cp.on ? t.o2s : t.o2, ao, out, C, sf, res));
  tfree(e, ao);
  return 0;
}

// patch_tokens: the block's tokens are numbered in patch order (sdm_common.h) between the GroupNorm in front of proj_in and the proj_out epilogue, and `bias` /
// `tiles` come in that order; everything in between is order-free (LayerNorm, the Linears, the softmax over keys, the shared cross-attention operand)
static int transformer(sdm_ctx* e, const TfB& t, const T& x, const T& uin, const CrossPlanes& cp, bool masked, const float* bias, const int* tiles, bool patch_tokens,
                       T* out) {
  const int sf = e->cfg.stream_f32;
  const int C = t.C, L = x.H * x.W;
  T hn, h, n, qkv, ao, h2, f;
  const int pf = unet_attn_plane_fmt(e);                        // plane format of q | k | v; SDM_ATTN_PV_SPLIT=1 (fully split P.V, test hook) needs V_lo too
  const int pa = pf ? 1 : 0;                                   // split-precision attention cores: q|k|v as hi|lo planes
  const bool need_vlo = pf == 2 && opt("attn_pv_split") != 0;
  // plane-fed GEMMs (k_gemm.h): every Linear of the block takes a P3 operand written by its producer - GroupNorm apply, LayerNorm, the GEGLU and
  // ff.net.2 epilogues - or, behind the attention cores (fp32 output), by one conversion pass
  const bool p3 = transformer_p3(e, t, pf);
  const int nf = p3 ? kFmtP3 : -1;                             // operand format of the norms' outputs (-1: the engine's activation type)
  const bool p3a = p3 && L % 32 == 0 && opt("gemm_p3_attn") != 0;                           // the attention cores write the planes themselves (O^T accumulators = the GEMM's operand layout)
  auto attn_out = [&](T& a) -> int {                           // the attention output as the next GEMM's operand
    if (!p3 || p3a) return 0;
    T ap;
    TRY(op_to_p3(e, a, &ap));
    tfree(e, a);
    a = ap;
    return 0;
  };
  if (patch_tokens && !(p3 && sdm_patch_tokens_ok(x.H, x.W))) SDM_FAIL(e, SDM_ERR_STATE, "transformer: patch token order without the plane-fed GEMMs");
  TRY(op_gn(e, e->norms[t.gn], x, nullptr, 0, e->cfg.unet_tf_gn_eps, &hn, nf, patch_tokens));
  TRY(linear(e, t.proj_in, hn, &h, C, sf));
  tfree(e, hn);
  // self-attention with the trimap key bias
  TRY(op_ln(e, e->norms[t.ln1], h, e->cfg.unet_ln_eps, &n, nf));
  TRY(linear(e, t.qkv1, n, &qkv, 3 * C, pf, nullptr, false, need_vlo ? -1 : 2 * C));
  tfree(e, n);
  ao = talloc(e, x.N, x.H, x.W, C, p3a ? kFmtP3 : e->act_f32);
  {
    const half_t* q = (const half_t*)qkv.p;
    AttnPrec ap; ap.prec = pa ? pf - 1 : 0; ap.out_f32 = p3a ? 1 : ao.f32; ap.out_p3 = p3a ? 1 : 0; ap.has_bias = ap.has_tiles = masked;
    ap.q_lo = ap.k_lo = ap.v_lo = (long)qkv.rows() * qkv.C;
    TRY(op_attention_raw(e, q, 3 * C, q ? q + C : nullptr, 3 * C, q ? q + 2 * C : nullptr, 3 * C, bias, x.N, t.heads, L, L, 64, ao.p, C, true, tiles, ap));
  }
  tfree(e, qkv);
  TRY(attn_out(ao));
  TRY(linear(e, t.o1, ao, &h2, C, sf, &h));
  tfree(e, ao); tfree(e, h);
  // cross-attention to the trimap-latent tokens
  TRY(op_ln(e, e->norms[t.ln2], h2, e->cfg.unet_ln_eps, &n, nf));
  TRY(cross_attention(e, t, n, uin, cp, pf, p3, p3a, &h2, &h));
  tfree(e, h2);
  // GEGLU feed-forward
  TRY(op_ln(e, e->norms[t.ln3], h, e->cfg.unet_ln_eps, &n, nf));
  TRY(linear(e, t.ff1, n, &f, 4 * C, p3 ? kFmtP3 : e->act_f32));
  tfree(e, n);
  // (P3: h2 only feeds proj_out - whose fused statistics need image-aligned row tiles on whole 32-row blocks; otherwise proj_out keeps the fp32 kernel)
  TRY(linear(e, t.ff2, f, &h2, C, (p3 && L % 32 == 0) ? kFmtP3 : sf, &h));
  tfree(e, f); tfree(e, h);
  TRY(linear(e, t.proj_out, h2, out, C, sf, &x, true, -1, patch_tokens));
  tfree(e, h2);
  return 0;
}

// ------------------------------------------------------------------------------------------------
// embedding constants (host): emb = time_embedding(time_proj(trans)) + bbox_embedding(sincos(coords))
//   replace.py:419-459; each ResBlock adds time_emb_proj(silu(emb)) after conv1 (Appendix A.3) -> folded
//   into that conv's bias table, one row per (trans, coords) variant.
// ------------------------------------------------------------------------------------------------
static void sincos_embed(float t, int dim, float* out) {  // get_timestep_embedding(flip_sin_to_cos=True, shift=0)
  const int half = dim / 2;
  for (int i = 0; i < half; ++i) {
    const float f = expf(-logf(10000.0f) * (float)i / (float)half);
    const float a = t * f;
    out[i] = cosf(a);
    out[half + i] = sinf(a);
  }
  if (dim & 1) out[dim - 1] = 0.0f;                       // odd dim: diffusers pads one zero column
}
// meta_arch.py:153-162: N point coordinates are zero-padded to the first i >= N that divides the point-embedding input
// dim P (1680 in the reference), each padded value is embedded with P / i channels.  Returns 0 if no such i < P exists
// (the reference's loop would fall through with unbound variables).
static int point_pad_len(int N, int P) {
  for (int i = N; i < P; ++i)
    if (i > 0 && P % i == 0) return i;
  return 0;
}
static void host_linear(const float* W, const float* b, const float* x, int O, int I, float* y) {
  for (int o = 0; o < O; ++o) {
    double acc = b ? (double)b[o] : 0.0;
    const float* w = W + (size_t)o * I;
    for (int i = 0; i < I; ++i) acc += (double)w[i] * (double)x[i];
    y[o] = (float)acc;
  }
}
static inline float host_silu(float x) { return x / (1.0f + expf(-x)); }

static int compute_variant_tables(sdm_ctx* e, int vidx) {
  const Variant& v = e->variants[vidx];
  const sdm_config& c = e->cfg;
  const int c0 = c.unet_channels[0], te = c0 * 4, bd = c.bbox_embeddings_input_dim;
  const float* H = e->hostblob.data();
  std::vector<float> tp(c0), t1(te), op(te), ce(bd), b1(te), aug(te), se(te);
  sincos_embed((float)v.trans, c0, tp.data());
  host_linear(H + e->h_time1w, H + e->h_time1b, tp.data(), te, c0, t1.data());
  for (auto& x : t1) x = host_silu(x);
  host_linear(H + e->h_time2w, H + e->h_time2b, t1.data(), te, te, op.data());
  if (v.kind == 0) {          // box prompt: 4 coordinates x (bd/4) channels -> bbox_embedding (meta_arch.py:178-187, replace.py:451-455)
    for (int k = 0; k < 4; ++k) sincos_embed(v.c[k], bd / 4, ce.data() + k * (bd / 4));
    host_linear(H + e->h_bbox1w, H + e->h_bbox1b, ce.data(), te, bd, b1.data());
    for (auto& x : b1) x = host_silu(x);
    host_linear(H + e->h_bbox2w, H + e->h_bbox2b, b1.data(), te, te, aug.data());
  } else {                    // point prompt: padded coordinates x (P/i) channels -> point_embedding (meta_arch.py:153-176, replace.py:446-450)
    const int P = c.point_embeddings_input_dim, npad = point_pad_len((int)v.c.size(), P), ch = P / npad;
    std::vector<float> pe((size_t)P, 0.0f);
    for (int k = 0; k < npad; ++k) sincos_embed(k < (int)v.c.size() ? v.c[k] : 0.0f, ch, pe.data() + (size_t)k * ch);
    host_linear(H + e->h_point1w, H + e->h_point1b, pe.data(), te, P, b1.data());
    for (auto& x : b1) x = host_silu(x);
    host_linear(H + e->h_point2w, H + e->h_point2b, b1.data(), te, te, aug.data());
  }
  for (int i = 0; i < te; ++i) se[i] = host_silu(op[i] + aug[i]);
  std::vector<float> row;
  for (auto& t : e->tembs) {
    row.assign(t.cout_pad, 0.0f);
    host_linear(H + t.w_hoff, H + t.b_hoff, se.data(), t.cout, te, row.data());
    for (int o = 0; o < t.cout; ++o) row[o] += H[t.cb_hoff + o];
    SDM_CHECK_DEV(e, dev_memcpy_h2d(t.table + (size_t)vidx * t.cout_pad, row.data(), (size_t)t.cout_pad * 4, e->stream));
    SDM_CHECK_DEV(e, dev_sync(e->stream));   // `row` is reused
  }
  return 0;
}

static int prepare_variants(sdm_ctx* e, int B, const int32_t* is_trans, const float* cond, int cond_dim, int cond_kind) {
  std::vector<int> sel(B);
  std::vector<Variant> want(B);
  if (cond_kind == 1) {
    if (!cond || cond_dim <= 0 || point_pad_len(cond_dim, e->cfg.point_embeddings_input_dim) == 0)
      SDM_FAIL(e, SDM_ERR_INVALID, "point prompt: %d coordinates cannot be padded to a divisor of %d", cond_dim, e->cfg.point_embeddings_input_dim);
  } else if (cond && cond_dim != 4) {
    SDM_FAIL(e, SDM_ERR_INVALID, "box prompt: expected 4 coordinates per image, got %d", cond_dim);
  }
  for (int b = 0; b < B; ++b) {
    want[b].trans = 1 - (is_trans ? (int)is_trans[b] : 0);        // meta_arch.py:237-238
    want[b].kind = cond_kind;
    if (cond_kind == 1) {
      want[b].c.assign(cond + (size_t)b * cond_dim, cond + (size_t)(b + 1) * cond_dim);
    } else {
      const float def[4] = {0.f, 0.f, 1.f, 1.f};                  // sdmatte_nodes.py:353 / meta_arch.py:189-190
      want[b].c.assign(4, 0.0f);
      for (int k = 0; k < 4; ++k) want[b].c[k] = cond ? cond[b * 4 + k] : def[k];
    }
  }
  auto find = [&](const Variant& v) {
    for (size_t i = 0; i < e->variants.size(); ++i)
      if (e->variants[i] == v) return (int)i;
    return -1;
  };
  {   // distinct conditionings of THIS batch; the tables hold at least that many rows (plus what is cached from earlier calls)
    std::vector<Variant> uniq;
    for (int b = 0; b < B; ++b) {
      bool seen = false;
      for (auto& u : uniq) if (u == want[b]) { seen = true; break; }
      if (!seen) uniq.push_back(want[b]);
    }
    int missing = 0;
    for (auto& u : uniq) if (find(u) < 0) ++missing;
    if ((int)e->variants.size() + missing > e->variant_cap) {
      // not enough rows: drop the cached rows (they are recomputed on demand) and, if this batch alone needs more, grow the tables
      e->variants.clear();
      if ((int)uniq.size() > e->variant_cap) {
        const int cap = std::max(rup((int)uniq.size(), 8), kMinVariantRows);
        SDM_CHECK_DEV(e, dev_sync(e->stream));
        for (auto& t : e->tembs) {
          if (t.table) dev_free(t.table);
          void* q = nullptr;
          if (dev_malloc(&q, (size_t)cap * t.cout_pad * 4) != 0) { t.table = nullptr; e->variant_cap = 0; SDM_FAIL(e, SDM_ERR_NOMEM, "cannot allocate %d conditioning rows", cap); }
          t.table = (float*)q;
        }
        e->variant_cap = cap;
      }
    }
    for (int b = 0; b < B; ++b) {
      int f = find(want[b]);
      if (f < 0) {
        e->variants.push_back(want[b]);
        f = (int)e->variants.size() - 1;
        TRY(compute_variant_tables(e, f));
      }
      sel[b] = f;
    }
  }
  if (B > e->bias_sel_cap) {
    if (e->d_bias_sel) dev_free(e->d_bias_sel);
    SDM_CHECK_DEV(e, dev_malloc((void**)&e->d_bias_sel, (size_t)B * 4));
    e->bias_sel_cap = B;
  }
  SDM_CHECK_DEV(e, dev_memcpy_h2d(e->d_bias_sel, sel.data(), (size_t)B * 4, e->stream));
  SDM_CHECK_DEV(e, dev_sync(e->stream));
  return 0;
}

// ------------------------------------------------------------------------------------------------
// the model: x16 [2B,SH,SW,16] fp16 (rgb images then trimaps), plane [B,SH,SW] fp32 (trimap in [-1,1]) -> alpha [B,SH,SW]
// ------------------------------------------------------------------------------------------------
// plane (optional): the trimap plane [B][H][W] behind images B .. 2B-1 of x16 - those images are piecewise constant, and the encoder's wide convs do
// not multiply the output tiles that lie inside one region (k_misc.h cmask_*, op_conv; engine option trimap_skip; split-precision mode only: the F8
// kernel is the one that knows how to leave tiles out)
static int vae_encode(sdm_ctx* e, const T& x16, T* moments, const T* plane = nullptr) {
  const float eps = e->cfg.vae_eps;
  T h, t;
  T xin = x16;
  const bool cm = plane && opt("trimap_skip") != 0 && e->act_f32 && x16.N == 2 * plane->N && plane->H == x16.H && plane->W == x16.W;
  if (cm) {
    const long hw = (long)x16.H * x16.W;
    T mb = talloc(e, 1, 1, 1, (int)(((size_t)x16.N * hw + 3) / 4), 1);
    xin.cmask = (unsigned char*)mb.p; xin.cm_off = mb.off; xin.cm_bytes = mb.bytes; xin.cm_n0 = plane->N;
    T tab = talloc(e, 1, 1, 1, x16.N * 4, 1);
    if (!e->dry) {
      SDM_LAUNCH(cmask_table_kernel, dim3((unsigned)plane->N), dim3(256), 0, e->stream, (const float*)plane->p, (unsigned int*)tab.p, plane->N, x16.H, x16.W);
      SDM_LAUNCH(cmask_init_kernel, dim3((unsigned)((plane->N * hw + 255) / 256)), dim3(256), 0, e->stream, (const float*)plane->p, xin.cmask, (const unsigned int*)tab.p,
                 plane->N, plane->N, hw);
    }
    tfree(e, tab);
  }
  TRY(conv_simple(e, e->enc_conv_in, xin, &h, e->cfg.vae_channels[0], e->cfg.stream_f32, 1, 0, 0, nullptr, 1.0f, true));
  if (cm) tfree_raw(e, xin.cm_off, xin.cm_bytes);
  for (int i = 0; i < 4; ++i) {
    for (auto& r : e->enc_res[i]) { TRY(resblock(e, r, h, nullptr, eps, &t)); tfree(e, h); h = t; }
    if (i < 3) { TRY(conv_simple(e, e->enc_down[i], h, &t, e->cfg.vae_channels[i], e->cfg.stream_f32, 2, 1, 0, nullptr, 1.0f, true)); tfree(e, h); h = t; }
  }
  TRY(resblock(e, e->enc_mid0, h, nullptr, eps, &t)); tfree(e, h); h = t;
  TRY(vae_attention(e, e->enc_attn, h, &t)); tfree(e, h); h = t;
  TRY(resblock(e, e->enc_mid1, h, nullptr, eps, &t)); tfree(e, h); h = t;
  *moments = talloc(e, h.N, h.H, h.W, 16, e->act_f32);
  { ConvArgs a; a.out = moments; TRY(gn_conv(e, e->norms[e->enc_norm_out], e->convs[e->enc_conv_out], h, nullptr, 1, eps, a)); }
  tfree(e, h);
  return 0;
}

static int vae_decode(sdm_ctx* e, const T& z, T* dec) {
  const float eps = e->cfg.vae_eps;
  T h, t;
  TRY(conv_simple(e, e->dec_conv_in, z, &h, e->cfg.vae_channels[3], e->cfg.stream_f32, 1, 0, 0, nullptr, 1.0f, true));
  TRY(resblock(e, e->dec_mid0, h, nullptr, eps, &t)); tfree(e, h); h = t;
  TRY(vae_attention(e, e->dec_attn, h, &t)); tfree(e, h); h = t;
  TRY(resblock(e, e->dec_mid1, h, nullptr, eps, &t)); tfree(e, h); h = t;
  for (int i = 0; i < 4; ++i) {
    for (auto& r : e->dec_res[i]) { TRY(resblock(e, r, h, nullptr, eps, &t)); tfree(e, h); h = t; }
    if (i < 3) { TRY(conv_simple(e, e->dec_up[i], h, &t, e->cfg.vae_channels[3 - i], e->cfg.stream_f32, 1, 0, 1, nullptr, 1.0f, true)); tfree(e, h); h = t; }
  }
  *dec = talloc(e, h.N, h.H, h.W, 4, 1);
  { ConvArgs a; a.out = dec; TRY(gn_conv(e, e->norms[e->dec_norm_out], e->convs[e->dec_conv_out], h, nullptr, 1, eps, a)); }
  tfree(e, h);
  return 0;
}

// Does U-Net level k (latent H x W) run its transformers in patch token order?  The option, the rule of the shape, and every transformer of the level on the
// plane-fed GEMMs (the two kernels that carry the map).  Decided once per forward in run_model, for the level's key bias and its transformers alike.
static bool level_patch_tokens(sdm_ctx* e, int k, int H, int W, bool option_on) {
  if (!option_on || !sdm_patch_tokens_ok(H, W)) return false;
  const int pf = unet_attn_plane_fmt(e);
  bool ok = true;
  if (k < 3) for (auto& t : e->u_down_tf[k]) ok = ok && transformer_p3(e, t, pf);
  if (k == 3) ok = ok && transformer_p3(e, e->u_midtf, pf);
  if (k < 3) for (auto& t : e->u_up_tf[3 - k]) ok = ok && transformer_p3(e, t, pf);
  return ok;
}

static int unet_forward(sdm_ctx* e, const T& uin, bool masked, float* const* bias_lvl, int* const* tiles_lvl, const bool* patch_lvl, T* out) {
  const sdm_config& c = e->cfg;
  const float eps = c.unet_res_eps;
  const int sf = c.stream_f32;
  std::vector<T> skips;
  T h, t;
  CrossPlanes cp;
  TRY(cross_planes_build(e, uin, &cp));
  TRY(conv_simple(e, e->u_conv_in, uin, &h, c.unet_channels[0], sf, 1, 0, 0, nullptr, 1.0f, true));
  skips.push_back(h);
  for (int i = 0; i < 4; ++i) {
    for (size_t j = 0; j < e->u_down_res[i].size(); ++j) {
      TRY(resblock(e, e->u_down_res[i][j], h, nullptr, eps, &t));
      if (i < 3) {
        T t2;
        TRY(transformer(e, e->u_down_tf[i][j], t, uin, cp, masked, bias_lvl[i], tiles_lvl[i], patch_lvl[i], &t2));
        tfree(e, t); t = t2;
      }
      h = t;                       // previous h stays alive as a skip
      skips.push_back(h);
    }
    if (i < 3) {
      TRY(conv_simple(e, e->u_down_ds[i], h, &t, c.unet_channels[i], sf, 2, 0, 0, nullptr, 1.0f, true));
      h = t;
      skips.push_back(h);
    }
  }
  // mid (h aliases the last skip: do not free it here)
  TRY(resblock(e, e->u_mid0, h, nullptr, eps, &t)); h = t;
  TRY(transformer(e, e->u_midtf, h, uin, cp, masked, bias_lvl[3], tiles_lvl[3], patch_lvl[3], &t)); tfree(e, h); h = t;
  TRY(resblock(e, e->u_mid1, h, nullptr, eps, &t)); tfree(e, h); h = t;
  for (int i = 0; i < 4; ++i) {
    for (size_t j = 0; j < e->u_up_res[i].size(); ++j) {
      T s = skips.back(); skips.pop_back();
      TRY(resblock(e, e->u_up_res[i][j], h, &s, eps, &t));   // cat([h, skip], dim=1) then ResBlock (replace.py:509-536)
      tfree(e, h); tfree(e, s); h = t;
      if (i > 0) {
        TRY(transformer(e, e->u_up_tf[i][j], h, uin, cp, masked, bias_lvl[3 - i], tiles_lvl[3 - i], patch_lvl[3 - i], &t));
        tfree(e, h); h = t;
      }
    }
    if (i < 3) { TRY(conv_simple(e, e->u_up_us[i], h, &t, c.unet_channels[3 - i], sf, 1, 0, 1, nullptr, 1.0f, true)); tfree(e, h); h = t; }
  }
  // label_latent / scaling_factor (meta_arch.py:254) folded into the conv_out epilogue
  *out = talloc(e, h.N, h.H, h.W, 16, e->act_f32);
  { ConvArgs a; a.out = out; a.out_scale = 1.0f / c.vae_scaling_factor; TRY(gn_conv(e, e->norms[e->u_norm_out], e->convs[e->u_conv_out], h, nullptr, 1, eps, a)); }
  tfree(e, h);
  cross_planes_free(e, &cp);
  return 0;
}

static int run_model(sdm_ctx* e, const T& x16, const T& plane, int B, int SH, int SW, bool use_mask, T* alpha) {
  const sdm_config& c = e->cfg;
  const int lh = SH / 8, lw = SW / 8;
  // attention key bias at the 4 U-Net levels (meta_arch.py:200-204, replace.py:401-403,56-63)
  T biasbuf[4], tilebuf[4];
  float* bias_lvl[4];
  int* tiles_lvl[4];            // per level: the key tiles that can contribute to the softmax (AttnParams::tiles), built once per forward
  bool patch_lvl[4];            // per level: tokens in patch order (the bias is written in the order the level's transformers number their tokens)
  const bool patch_opt = opt("attn_patch_tokens") != 0;
  for (int k = 0; k < 4; ++k) {
    const int lk2 = (lh >> k) * (lw >> k), nt = sdm_cdiv(lk2, 64);
    patch_lvl[k] = level_patch_tokens(e, k, lh >> k, lw >> k, patch_opt);
    biasbuf[k] = talloc(e, B, 1, 1, lk2, 1);
    tilebuf[k] = talloc(e, B, 1, 1, nt + 1, 1);
    bias_lvl[k] = (float*)biasbuf[k].p;
    tiles_lvl[k] = (int*)tilebuf[k].p;
    if (!e->dry && use_mask) {
      SDM_LAUNCH(mask_bias_kernel, dim3(sdm_cdiv(B * lk2, 256)), dim3(256), 0, e->stream, (const float*)plane.p, bias_lvl[k], B, SH, SW, k,
                 c.attn_mask_value, SDM_LOG2E, patch_lvl[k] ? 1 : 0);
      SDM_LAUNCH(attn_active_tiles_kernel, dim3(B), dim3(256), 0, e->stream, (const float*)bias_lvl[k], lk2, nt, tiles_lvl[k], nt + 1,
                 SDM_ATTN_SKIP_MARGIN);
    }
    // prompt types outside attn_mask_aux_input run the self-attention without a key mask (meta_arch.py:199-206)
    if (!use_mask) { bias_lvl[k] = nullptr; tiles_lvl[k] = nullptr; }
  }
  // VAE encode of rgb and trimap as one batch (meta_arch.py:139-145, 209-212)
  T moments;
  TRY(vae_encode(e, x16, &moments, &plane));
  // quant_conv -> mean half * scaling_factor, written straight into the 8(+8 pad)-channel U-Net input:
  // channels 0..3 = rgb latent, 4..7 = trimap latent (torch.cat order of meta_arch.py:244)
  T uin = talloc(e, B, lh, lw, 16, e->act_f32);
  if (!e->dry) SDM_CHECK_DEV(e, dev_memset(uin.p, 0, uin.bytes, e->stream));
  for (int half = 0; half < 2; ++half) {
    T mv = moments; mv.N = B;
    if (!e->dry) mv.p = (unsigned char*)moments.p + (size_t)half * B * lh * lw * 16 * fmt_bytes(moments.f32);
    ConvArgs a; a.in0 = &mv; a.out = &uin; a.out_ch_off = half * 4; a.cout_valid = 4; a.out_scale = c.vae_scaling_factor;
    TRY(op_conv(e, e->convs[e->quant], a));
  }
  tfree(e, moments);
  // cross-attention context (meta_arch.py:215-218: aux_conv_in(trimap latent) as [B, l*l, ctx]) is never materialised:
  // every block's K|V comes straight from the latent through the folded 3x3 conv (transformer())
  T lat;
  TRY(unet_forward(e, uin, use_mask, bias_lvl, tiles_lvl, patch_lvl, &lat));
  tfree(e, uin);
  for (int k = 3; k >= 0; --k) { tfree(e, tilebuf[k]); tfree(e, biasbuf[k]); }
  // post_quant_conv + decoder (meta_arch.py:255-256)
  T z;
  TRY(conv_simple(e, e->post_quant, lat, &z, 16, e->act_f32)); tfree(e, lat);
  T dec;
  TRY(vae_decode(e, z, &dec)); tfree(e, z);
  *alpha = talloc(e, B, SH, SW, 1, 1);
  if (!e->dry)
    SDM_LAUNCH(alpha_out_kernel, dim3((unsigned)(((long)B * SH * SW + 255) / 256)), dim3(256), 0, e->stream, (const float*)dec.p, (float*)alpha->p,
               (long)B * SH * SW);
  tfree(e, dec);
  return 0;
}

// ------------------------------------------------------------------------------------------------
// trimap from a mask (k_trimap.h): mask fp32 [B,H,W] -> the signed column-distance plane (int16 [B,H,W]) -> trimap fp32 [B,H,W]
// ------------------------------------------------------------------------------------------------
static int trimap_check(sdm_ctx* e, int B, int H, int W, int erode_px, int dilate_px) {
  if (B <= 0 || H <= 0 || W <= 0) SDM_FAIL(e, SDM_ERR_INVALID, "trimap from mask: bad mask size %dx%dx%d", B, H, W);
  if (erode_px < 0 || erode_px > SDM_TRIMAP_MAX_RADIUS || dilate_px < 0 || dilate_px > SDM_TRIMAP_MAX_RADIUS)
    SDM_FAIL(e, SDM_ERR_INVALID, "trimap from mask: erode_px = %d, dilate_px = %d outside 0 .. %d", erode_px, dilate_px, SDM_TRIMAP_MAX_RADIUS);
  // one row-kernel block per 256-pixel row segment, in a 1-D grid
  if ((double)B * H * sdm_cdiv(W, SDM_TRIMAP_ROWS_W) >= 2147483647.0) SDM_FAIL(e, SDM_ERR_INVALID, "trimap from mask: %dx%dx%d is too large", B, H, W);
  return 0;
}

// rows per block of the column kernel: tall blocks re-read the least halo, short ones fill the chip at small sizes and keep the LDS under 48 KB
static int trimap_cols_rows(int B, int H, int W, int R) {
  int rows = 128;
  while (rows > 32 && ((long)B * sdm_cdiv(H, rows) * sdm_cdiv(W, SDM_TRIMAP_COLS_W) < 512 || trimap_cols_smem(rows, R) > 48 * 1024)) rows /= 2;
  return rows;
}

static void op_trimap(sdm_ctx* e, const float* mask, int B, int H, int W, float threshold, int erode_px, int dilate_px, short* plane, float* trimap) {
  const int R = std::max(erode_px, dilate_px), rows = trimap_cols_rows(B, H, W, R);
  const double px = (double)B * H * W;
  prof_begin(e, "trimap_cols", 0, px * 6);
  count_kernel("trimap_cols");
  SDM_LAUNCH(trimap_cols_kernel, dim3((unsigned)(B * sdm_cdiv(H, rows) * sdm_cdiv(W, SDM_TRIMAP_COLS_W))), dim3(256), trimap_cols_smem(rows, R), e->stream, mask, plane,
             B, H, W, threshold, R, rows);
  prof_end(e);
  prof_begin(e, "trimap_rows", 0, px * 6);
  count_kernel("trimap_rows");
  SDM_LAUNCH(trimap_rows_kernel, dim3((unsigned)((long)B * H * sdm_cdiv(W, SDM_TRIMAP_ROWS_W))), dim3(256), 0, e->stream, (const short*)plane, trimap, B, H, W,
             erode_px, dilate_px);
  prof_end(e);
}

// ------------------------------------------------------------------------------------------------
// the subject's box (k_roi.h): plane fp32 [B,H,W] -> raw extrema int32 [B,4] -> roi int32 [B,4] = {y0, x0, h, w}
// ------------------------------------------------------------------------------------------------
static int roi_check(sdm_ctx* e, const char* what, int B, int H, int W, float roi_threshold, int margin_px, int margin_pct, int square) {
  if (B <= 0 || H < 1 || W < 1) SDM_FAIL(e, SDM_ERR_INVALID, "%s: bad plane size %dx%dx%d", what, B, H, W);
  // pixel indices inside an image are ints
  if (H > SDM_FG_MAX_SIDE || W > SDM_FG_MAX_SIDE || (double)B * H * W > (double)SDM_FG_MAX_PIXELS)
    SDM_FAIL(e, SDM_ERR_INVALID, "%s: %dx%dx%d is too large (sides up to %d, %d pixels in all)", what, B, H, W, SDM_FG_MAX_SIDE, SDM_FG_MAX_PIXELS);
  // at least 0, so that what the reduction reads beyond the image (-1) is outside U
  if (!std::isfinite(roi_threshold) || !(roi_threshold >= 0.0f) || !(roi_threshold < 1.0f))
    SDM_FAIL(e, SDM_ERR_INVALID, "%s: roi_threshold = %g must be a finite number in [0, 1)", what, (double)roi_threshold);
  if (margin_px < 0 || margin_px > SDM_ROI_MAX_MARGIN_PX) SDM_FAIL(e, SDM_ERR_INVALID, "%s: margin_px = %d outside 0 .. %d", what, margin_px, SDM_ROI_MAX_MARGIN_PX);
  if (margin_pct < 0 || margin_pct > 100) SDM_FAIL(e, SDM_ERR_INVALID, "%s: margin_pct = %d outside 0 .. 100", what, margin_pct);
  if (square != 0 && square != 1) SDM_FAIL(e, SDM_ERR_INVALID, "%s: square = %d must be 0 or 1", what, square);
  return 0;
}

static bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// three launches, whatever the arguments
static void op_roi_box(sdm_ctx* e, const float* plane, int B, int H, int W, float roi_threshold, int margin_px, int margin_pct, int square, int* raw, int* roi) {
  prof_begin(e, "roi_init", 0, (double)B * 16);
  count_kernel("roi_init");
  SDM_LAUNCH(roi_init_kernel, dim3((unsigned)sdm_cdiv(B * 4, 256)), dim3(256), 0, e->stream, raw, B);
  prof_end(e);
  const dim3 grid((unsigned)(B * sdm_cdiv(H * W, SDM_ROI_PX)));
  prof_begin(e, "roi_reduce", 0, (double)B * H * W * 4);
  count_kernel("roi_reduce");
  if (W % 4 == 0 && aligned16(plane)) SDM_LAUNCH((roi_reduce_kernel<true>), grid, dim3(256), 0, e->stream, plane, raw, B, H, W, roi_threshold);
  else SDM_LAUNCH((roi_reduce_kernel<false>), grid, dim3(256), 0, e->stream, plane, raw, B, H, W, roi_threshold);
  prof_end(e);
  prof_begin(e, "roi_finalize", 0, (double)B * 32);
  count_kernel("roi_finalize");
  SDM_LAUNCH(roi_finalize_kernel, dim3((unsigned)sdm_cdiv(B, 64)), dim3(64), 0, e->stream, (const int*)raw, roi, B, H, W, margin_px, margin_pct, square);
  prof_end(e);
}

// ------------------------------------------------------------------------------------------------
// the distance field (k_distance.h): plane fp32 [B,H,W] -> class words -> carries -> column distances uint16 [B,H,W] -> the row pass, which writes
// the field (mode 0), the offset mask (mode 1) or the outlined cut-out (mode 2)
// ------------------------------------------------------------------------------------------------
static int df_check(sdm_ctx* e, const char* what, int B, int H, int W, float threshold) {
  if (B <= 0 || H < 1 || W < 1) SDM_FAIL(e, SDM_ERR_INVALID, "%s: bad plane size %dx%dx%d", what, B, H, W);
  if (H > SDM_FG_MAX_SIDE || W > SDM_FG_MAX_SIDE || (double)B * H * W > (double)SDM_FG_MAX_PIXELS)
    SDM_FAIL(e, SDM_ERR_INVALID, "%s: %dx%dx%d is too large (sides up to %d, %d pixels in all)", what, B, H, W, SDM_FG_MAX_SIDE, SDM_FG_MAX_PIXELS);
  if (!std::isfinite(threshold) || !(threshold >= 0.0f) || !(threshold < 1.0f))
    SDM_FAIL(e, SDM_ERR_INVALID, "%s: threshold = %g must be a finite number in [0, 1)", what, (double)threshold);
  return 0;
}

struct DfScratch { T bits, carry, cols; };
static DfScratch df_talloc(sdm_ctx* e, int B, int H, int W) {
  const int nt = sdm_cdiv(H, SDM_DF_TILE);
  DfScratch s;
  s.bits = talloc(e, B, nt, W, 1, 1);
  s.carry = talloc(e, B, nt, W, 4, 1);
  s.cols = talloc(e, B, H, W, 1, 0);      // (2 bytes per pixel)
  return s;
}
static void df_tfree(sdm_ctx* e, DfScratch& s) { tfree(e, s.cols); tfree(e, s.carry); tfree(e, s.bits); }

// four launches, whatever the arguments: df_bits, df_carry, df_cols and the row pass under the name of its mode (df_rows, df_offset, df_outline)
static void op_distance(sdm_ctx* e, const float* plane, int B, int H, int W, float threshold, DfScratch& s, int mode, const DfEmit& emit) {
  static_assert(SDM_DF_FIELD_NONE == SDM_DF_NONE && SDM_FG_MAX_SIDE <= 32768, "distance field limits");
  const int nt = sdm_cdiv(H, SDM_DF_TILE);
  const double px = (double)B * H * W, words = (double)B * nt * W;
  const dim3 tiles((unsigned)(B * nt * sdm_cdiv(W, 256)));
  prof_begin(e, "df_bits", 0, px * 4 + words * 4);
  count_kernel("df_bits");
  SDM_LAUNCH(df_bits_kernel, tiles, dim3(256), 0, e->stream, plane, (unsigned int*)s.bits.p, B, H, W, threshold);
  prof_end(e);
  prof_begin(e, "df_carry", 0, words * 24);      // the words twice, four carries
  count_kernel("df_carry");
  SDM_LAUNCH(df_carry_kernel, dim3((unsigned)sdm_cdiv(B * W, 256)), dim3(256), 0, e->stream, (const unsigned int*)s.bits.p, (int*)s.carry.p, B, H, W);
  prof_end(e);
  prof_begin(e, "df_cols", 0, words * 20 + px * 2);
  count_kernel("df_cols");
  SDM_LAUNCH(df_cols_kernel, tiles, dim3(256), 0, e->stream, (const unsigned int*)s.bits.p, (const int*)s.carry.p, (unsigned short*)s.cols.p, B, H, W);
  prof_end(e);
  const size_t smem = df_rows_smem(W);
  const dim3 rows((unsigned)(B * H));
  const unsigned short* cols = (const unsigned short*)s.cols.p;
  // per pixel: the column distance (2 bytes) and what the mode reads and writes
  if (mode == 0) {
    if (smem > 48 * 1024) SDM_SET_SMEM((df_rows_kernel<0>), df_rows_smem(SDM_FG_MAX_SIDE));
    prof_begin(e, "df_rows", 0, px * 6);
    count_kernel("df_rows");
    SDM_LAUNCH((df_rows_kernel<0>), rows, dim3(256), smem, e->stream, cols, B, H, W, emit);
  } else if (mode == 1) {
    if (smem > 48 * 1024) SDM_SET_SMEM((df_rows_kernel<1>), df_rows_smem(SDM_FG_MAX_SIDE));
    prof_begin(e, "df_offset", 0, px * 6);
    count_kernel("df_offset");
    SDM_LAUNCH((df_rows_kernel<1>), rows, dim3(256), smem, e->stream, cols, B, H, W, emit);
  } else {
    if (smem > 48 * 1024) SDM_SET_SMEM((df_rows_kernel<2>), df_rows_smem(SDM_FG_MAX_SIDE));
    prof_begin(e, "df_outline", 0, px * 34);
    count_kernel("df_outline");
    SDM_LAUNCH((df_rows_kernel<2>), rows, dim3(256), smem, e->stream, cols, B, H, W, emit);
  }
  prof_end(e);
}

// ------------------------------------------------------------------------------------------------
// top-level forward helpers
// ------------------------------------------------------------------------------------------------
static int ensure_buf(sdm_ctx* e, void** p, size_t* cap, size_t need) {
  if (*cap >= need) return 0;
  if (*p) { SDM_CHECK_DEV(e, dev_sync(e->stream)); dev_free(*p); *p = nullptr; *cap = 0; }
  SDM_CHECK_DEV(e, dev_malloc(p, need));
  *cap = need;
  return 0;
}

// mode 0: core API (NCHW preprocessed, S x S); mode 1: node API (BHWC image + BHW trimap at H x W)
// mode 0 takes the inference size as (SH, SW) = (H, W) and S is ignored; mode 1 resizes H x W to S x S like the node.
// node tail (mode 1 only): mask_refine + output composition on the GPU, sdmatte_nodes.py:365-397
// trimap_constraint stays a double up to the two thresholds: the reference compares fp32 tensors with the Python floats c and
// 1.0 - c (evaluated in double), i.e. with float32(c) and float32(1.0 - c) - for c = 0.8 the latter is 0.2f, not 1.0f - 0.8f
struct NodeTail {
  int output_mode = 0, mask_refine = 0; double c = 0.8; float* matted = nullptr; int TH = 0, TW = 0;
  // sdm_apply_matte_mask: the `trimap` argument of forward_impl is a mask, and the trimap is made from it on the device (op_trimap)
  bool from_mask = false; float threshold = 0.5f; int erode_px = 0, dilate_px = 0; float* trimap_out = nullptr;
  // sdm_apply_matte_roi: the model sees the box of the trimap (op_roi_box) instead of the frame; the box stays on the device
  bool roi = false; float roi_threshold = 0.0f; int margin_px = 0, margin_pct = 0, square = 0; int32_t* roi_out = nullptr;
  int channels() const { return output_mode == 1 ? 4 : 3; }
};

// One input or output of a product call: the caller's pointer and its size.  product_call replaces `p` by the device-side pointer - the same one
// for DEVICE pointers, its place in the I/O staging for HOST pointers - before the body runs.  An absent optional output has bytes == 0.
struct IoSpan { void* p; size_t bytes; };

// The scaffold of every product call (forward_impl, sdm_make_trimap, sdm_clean_mask, sdm_subject_roi, sdm_estimate_foreground, sdm_refine_alpha_guided, sdm_compose_canvas, sdm_distance_field, sdm_offset_mask, sdm_outline, sdm_smooth_alpha_temporal, sdm_smooth_alpha_motion, sdm_defocus_background, sdm_fill_background, sdm_harmonize, sdm_screen_colour, sdm_chroma_key, sdm_matte_metrics, sdm_band_tiles, sdm_apply_matte_tiles) around its body, the
// talloc / launch / tfree sequence that arena_two_pass runs twice.  The caller has checked its arguments.
// Stream contract (include/sdmatte.h): kernels run on the engine's own stream.  For DEVICE pointers the caller names the stream on which it
// produced the inputs and will consume the outputs (NULL = the device's default stream): the engine stream waits for everything queued there
// at call time, and that stream waits for the outputs before the call returns control (no host synchronisation).  HOST pointers are copied
// on the engine stream through the staging buffers io_in / io_out, packed back to back in list order (the body may pick a kernel by the
// alignment of what it is given), followed by a host sync.  The arena and the staging are what sdm_resident_bytes counts beside the weights.
template <size_t NI, size_t NO, typename F>
static int product_call(sdm_ctx* e, int ptr_kind, void* stream_arg, IoSpan (&in)[NI], IoSpan (&out)[NO], F body) {
  if (ptr_kind != SDM_PTR_HOST && ptr_kind != SDM_PTR_DEVICE)
    SDM_FAIL(e, SDM_ERR_INVALID, "unknown ptr_kind %d (SDM_PTR_HOST = %d or SDM_PTR_DEVICE = %d)", ptr_kind, SDM_PTR_HOST, SDM_PTR_DEVICE);
  OptReadLock opt_lock;          // kernel-selection options stay put for both passes of this call
  const bool host = ptr_kind == SDM_PTR_HOST;
  void* host_out[NO];
  if (host) {
    size_t in_bytes = 0, out_bytes = 0;
    for (const IoSpan& s : in) in_bytes += s.bytes;
    for (const IoSpan& s : out) out_bytes += s.bytes;
    TRY(ensure_buf(e, &e->io_in, &e->io_in_bytes, in_bytes));
    TRY(ensure_buf(e, &e->io_out, &e->io_out_bytes, out_bytes));
    unsigned char* d = (unsigned char*)e->io_in;
    for (IoSpan& s : in) { SDM_CHECK_DEV(e, dev_memcpy_h2d(d, s.p, s.bytes, e->stream)); s.p = d; d += s.bytes; }
    d = (unsigned char*)e->io_out;
    for (size_t i = 0; i < NO; ++i) { host_out[i] = out[i].p; if (out[i].bytes) out[i].p = d; d += out[i].bytes; }
  }
#ifndef SDM_EMU
  else {
    SDM_CHECK_DEV(e, (int)hipEventRecord(e->ev_in, (hipStream_t)stream_arg));
    SDM_CHECK_DEV(e, (int)hipStreamWaitEvent((hipStream_t)e->stream, e->ev_in, 0));
  }
#endif
  TRY(arena_two_pass(e, 0, true, body));
#ifndef SDM_EMU
  (void)hipEventRecord(e->ev1, (hipStream_t)e->stream);
#endif
  if (host) {
    for (size_t i = 0; i < NO; ++i)
      if (out[i].bytes) SDM_CHECK_DEV(e, dev_memcpy_d2h(host_out[i], out[i].p, out[i].bytes, e->stream));
    SDM_CHECK_DEV(e, dev_sync(e->stream));
  }
#ifndef SDM_EMU
  else {
    SDM_CHECK_DEV(e, (int)hipEventRecord(e->ev_out, (hipStream_t)e->stream));
    SDM_CHECK_DEV(e, (int)hipStreamWaitEvent((hipStream_t)stream_arg, e->ev_out, 0));
  }
#else
  (void)stream_arg;
#endif
  return 0;
}

static int forward_impl(sdm_ctx* e, int mode, const float* image, const float* trimap, int B, int H, int W, int S, const int32_t* is_trans,
                        const float* cond, int cond_dim, int cond_kind, bool use_mask, float* out, int ptr_kind, void* stream_arg,
                        const NodeTail* tail = nullptr) {
  if (!e->finalized) SDM_FAIL(e, SDM_ERR_STATE, "weights not finalised: call sdm_load_tensor(...) and sdm_finalize_weights first");
  const int SH = (mode == 0) ? H : S, SW = (mode == 0) ? W : S;
  if (B <= 0 || SH <= 0 || SW <= 0 || SH % 64 || SW % 64)
    SDM_FAIL(e, SDM_ERR_INVALID, "inference size must be a positive multiple of 64 (got %dx%d)", SH, SW);
  if (mode == 1 && (H <= 0 || W <= 0)) SDM_FAIL(e, SDM_ERR_INVALID, "bad image size %dx%d", H, W);
  // node API: the trimap may have its own size (the reference resizes image and trimap independently, sdmatte_nodes.py:212-214,349)
  const int TH = (tail && tail->TH > 0) ? tail->TH : H, TW = (tail && tail->TW > 0) ? tail->TW : W;
  const size_t in_tri = (size_t)B * TH * TW * 4;
  const size_t alpha_bytes = (size_t)B * H * W * 4;
  const bool from_mask = tail && tail->from_mask, roi = tail && tail->roi;
  IoSpan in[] = {{(void*)image, (size_t)B * H * W * 3 * 4},      // mode 0: [B,3,SH,SW]; mode 1: [B,H,W,3]
                 {(void*)trimap, in_tri}};
  IoSpan outs[] = {{out, alpha_bytes},                           // host hand-over: alpha, then the composed image
                   {tail ? tail->matted : nullptr, tail ? alpha_bytes * tail->channels() : 0},
                   // ... then the trimap made from the mask, if the caller wants it
                   {from_mask ? tail->trimap_out : nullptr, (from_mask && tail->trimap_out) ? in_tri : 0},
                   // ... then the box
                   {roi ? tail->roi_out : nullptr, (roi && tail->roi_out) ? (size_t)B * 16 : 0}};
  return product_call(e, ptr_kind, stream_arg, in, outs, [&]() -> int {
    const float* d_img = (const float*)in[0].p; const float* d_tri = (const float*)in[1].p;
    float* d_out = (float*)outs[0].p; float* d_matted = (float*)outs[1].p; float* d_tri_out = (float*)outs[2].p; int* d_roi_out = (int*)outs[3].p;
    if (e->dry) TRY(prepare_variants(e, B, is_trans, cond, cond_dim, cond_kind));      // once per call: behind the input copies, ahead of the launches
    T gtri;      // sdm_apply_matte_mask: the trimap of this call, made from the mask in d_tri; it stands in for d_tri from here on
    const float* tri_in = d_tri;
    if (from_mask) {
      T dist = talloc(e, B, TH, TW, 1, 0);      // (2 bytes per pixel: the signed column distances)
      gtri = talloc(e, B, TH, TW, 1, 1);
      if (!e->dry) {
        op_trimap(e, d_tri, B, TH, TW, tail->threshold, tail->erode_px, tail->dilate_px, (short*)dist.p, (float*)gtri.p);
        if (d_tri_out) SDM_CHECK_DEV(e, dev_memcpy_d2d(d_tri_out, gtri.p, in_tri, e->stream));
      }
      tfree(e, dist);
      tri_in = (const float*)gtri.p;
    }
    T box;       // sdm_apply_matte_roi: {y0, x0, h, w} per image, from the trimap of this call (TH x TW = H x W); read by the three resampling launches
    if (roi) {
      T raw = talloc(e, B, 1, 1, 4, 1);
      box = talloc(e, B, 1, 1, 4, 1);
      if (!e->dry) {
        op_roi_box(e, tri_in, B, H, W, tail->roi_threshold, tail->margin_px, tail->margin_pct, tail->square, (int*)raw.p, (int*)box.p);
        if (d_roi_out) SDM_CHECK_DEV(e, dev_memcpy_d2d(d_roi_out, box.p, (size_t)B * 16, e->stream));
      }
      tfree(e, raw);
    }
    T x16 = talloc(e, 2 * B, SH, SW, 16, e->act_f32);
    T plane = talloc(e, B, SH, SW, 1, 1);
    if (!e->dry) {
      const unsigned nb = (unsigned)(((long)B * SH * SW + 255) / 256);
      void* img16 = x16.p;
      void* tri16 = (unsigned char*)x16.p + (size_t)B * SH * SW * 16 * fmt_bytes(x16.f32);
      if (mode == 0) {
        SDM_LAUNCH(prep_nchw_kernel, dim3(nb), dim3(256), 0, e->stream, d_img, d_tri, img16, tri16, x16.f32, (float*)plane.p, B, SH, SW);
      } else if (roi) {
        // (an upper bound of the bytes: what is read depends on the box)
        prof_begin(e, "roi_prep_image", 0, (double)B * H * W * 12 + (double)B * S * S * 16 * fmt_bytes(x16.f32));
        count_kernel("roi_prep_image");
        SDM_LAUNCH(roi_prep_image_kernel, dim3(nb), dim3(256), 0, e->stream, d_img, (const int*)box.p, img16, x16.f32, B, H, W, S);
        prof_end(e);
        prof_begin(e, "roi_prep_trimap", 0, (double)B * H * W * 4 + (double)B * S * S * (16 * fmt_bytes(x16.f32) + 4));
        count_kernel("roi_prep_trimap");
        SDM_LAUNCH(roi_prep_trimap_kernel, dim3(nb), dim3(256), 0, e->stream, tri_in, (const int*)box.p, tri16, x16.f32, (float*)plane.p, B, H, W, S);
        prof_end(e);
      } else {
        SDM_LAUNCH(prep_image_kernel, dim3(nb), dim3(256), 0, e->stream, d_img, img16, x16.f32, B, H, W, S);
        SDM_LAUNCH(prep_trimap_kernel, dim3(nb), dim3(256), 0, e->stream, tri_in, tri16, x16.f32, (float*)plane.p, B, TH, TW, S);
      }
    }
    T alpha;
    TRY(run_model(e, x16, plane, B, SH, SW, use_mask, &alpha));
    if (!e->dry) {
      if (mode == 0) {
        SDM_CHECK_DEV(e, dev_memcpy_d2d(d_out, alpha.p, (size_t)B * SH * SW * 4, e->stream));
      } else {
        if (roi) {
          prof_begin(e, "roi_paste", 0, (double)B * H * W * 4 + (double)B * S * S * 4);
          count_kernel("roi_paste");
          SDM_LAUNCH(roi_paste_kernel, dim3((unsigned)(((long)B * H * W + 255) / 256)), dim3(256), 0, e->stream, (const float*)alpha.p, (const int*)box.p, d_out,
                     B, H, W, S);
          prof_end(e);
        } else {
          SDM_LAUNCH(resize_planes_kernel, dim3((unsigned)(((long)B * H * W + 255) / 256)), dim3(256), 0, e->stream, (const float*)alpha.p, d_out, B,
                     S, S, H, W, 1);
        }
        if (tail)
          SDM_LAUNCH(refine_compose_kernel, dim3((unsigned)(((long)B * H * W + 255) / 256)), dim3(256), 0, e->stream, d_img, tri_in, d_out, d_matted,
                     (long)B * H * W, tail->output_mode, tail->mask_refine, (float)tail->c, (float)(1.0 - tail->c));
      }
    }
    tfree(e, alpha); tfree(e, plane); tfree(e, x16); tfree(e, box); tfree(e, gtri);
    return 0;
  });
}

// runs an op outside forward(), for the hooks of sdm_hooks.h: no caller data to stage, an arena of 1 MB or more, a host sync at the end
template <typename F>
static int run_two_pass(sdm_ctx* e, F body) {
  OptReadLock opt_lock;          // (never nested: the product calls do not come through here)
  TRY(arena_two_pass(e, (size_t)1 << 20, false, [&]() -> int {
#ifdef SDM_EMU
    if (!e->dry && opt("emu_arena_extra")) {      // self-test of the check: one block the sizing pass did not make, ahead of the op's own
      const size_t b0 = (e->atrace.empty() ? 0 : e->atrace[0]) + 256;
      (void)talloc(e, 1, 1, 1, (int)(b0 / 4), 1);
    }
#endif
    return body();
  }));
  SDM_CHECK_DEV(e, dev_sync(e->stream));
  return 0;
}


// ------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------
static void load_ring_release(sdm_ctx* e);

extern "C" {

void sdm_default_config(sdm_config* c) {
  memset(c, 0, sizeof(*c));
  const int vc[4] = {128, 256, 512, 512}, uc[4] = {320, 640, 1280, 1280}, uh[4] = {5, 10, 20, 20};
  for (int i = 0; i < 4; ++i) { c->vae_channels[i] = vc[i]; c->unet_channels[i] = uc[i]; c->unet_heads[i] = uh[i]; }
  c->vae_layers_per_block = 2; c->unet_layers_per_block = 2;
  c->cross_attention_dim = 1024; c->unet_in_channels = 8; c->unet_out_channels = 4;
  c->bbox_embeddings_input_dim = 1280; c->point_embeddings_input_dim = 1680; c->groups = 32;
  c->vae_eps = 1e-6f; c->unet_res_eps = 1e-5f; c->unet_tf_gn_eps = 1e-6f; c->unet_ln_eps = 1e-5f;
  c->vae_scaling_factor = 0.18215f; c->attn_mask_value = -10000.0f;
  c->stream_f32 = 1;
  c->precise_mask = SDM_PRECISE_ALL;      // the precision that meets the 1e-3 parity bar (include/sdmatte.h); 0 selects the fast fp16-operand graph
}

int sdm_create(sdm_ctx** out, int device_id, const sdm_config* cfg) {
  if (!out) return SDM_ERR_INVALID;
  *out = nullptr;
#ifndef SDM_EMU
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    g_create_err = "no HIP device visible: the SDMatte engine is gfx950-only and has no CPU fallback";
    return SDM_ERR_NODEVICE;
  }
  if (device_id < 0 || device_id >= ndev) { g_create_err = "bad device id"; return SDM_ERR_INVALID; }
  if (hipSetDevice(device_id) != hipSuccess) { g_create_err = "hipSetDevice failed"; return SDM_ERR_HIP; }
#endif
  sdm_ctx* e = new sdm_ctx();
  if (cfg) e->cfg = *cfg; else sdm_default_config(&e->cfg);
  if (e->cfg.point_embeddings_input_dim <= 0) e->cfg.point_embeddings_input_dim = 1680;
  e->cfg.precise_mask &= SDM_PRECISE_ALL;
  if (opt("precise_mask") >= 0) e->cfg.precise_mask = opt("precise_mask") & SDM_PRECISE_ALL;      // experiment option (per-stage attribution)
  e->act_f32 = e->cfg.precise_mask ? 1 : 0;
  if (e->act_f32) e->cfg.stream_f32 = 1;
  e->device = device_id;
  const sdm_config& c = e->cfg;
  for (int i = 0; i < 4; ++i) {
    if (c.vae_channels[i] % 32 || c.unet_channels[i] % 64 || c.unet_heads[i] * 64 != c.unet_channels[i]) {
      g_create_err = "unsupported config: channels must be multiples of 32 (VAE) / 64 (U-Net) with head_dim 64";
      delete e; return SDM_ERR_INVALID;
    }
  }
  if (!(c.vae_channels[3] == 64 || c.vae_channels[3] == 512)) {
    g_create_err = "unsupported config: VAE mid channels must be 64 or 512 (single-head attention kernels)";
    delete e; return SDM_ERR_INVALID;
  }
  if (c.unet_in_channels > 16 || c.bbox_embeddings_input_dim % 8 || c.cross_attention_dim % 64) {
    g_create_err = "unsupported config"; delete e; return SDM_ERR_INVALID;
  }
  build_model(e);
#ifndef SDM_EMU
  hipStream_t st;
  if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) { g_create_err = "hipStreamCreate failed"; delete e; return SDM_ERR_HIP; }
  e->stream = st; e->own_stream = true;
  (void)hipEventCreate(&e->ev0); (void)hipEventCreate(&e->ev1);
  (void)hipEventCreateWithFlags(&e->ev_in, hipEventDisableTiming); (void)hipEventCreateWithFlags(&e->ev_out, hipEventDisableTiming);
#endif
  // weight arena (+ temb tables)
  void* p = nullptr;
  if (dev_malloc(&p, e->warena_bytes) != 0) { g_create_err = "cannot allocate weight arena"; sdm_destroy(e); return SDM_ERR_NOMEM; }
  e->warena = (unsigned char*)p;
  dev_memset(e->warena, 0, e->warena_bytes, e->stream);
  for (auto& L : e->convs) {
    L.w = (half_t*)(e->warena + L.w_off); L.b = (float*)(e->warena + L.b_off);
    if (L.split) L.w_lo = (half_t*)(e->warena + L.wlo_off);
    if (L.wdma_bytes) L.w_dma = (half_t*)(e->warena + e->canon_bytes + L.wdma_off);
    if (L.w3_bytes) L.w3 = e->warena + e->canon_bytes + L.w3_off;
    if (L.wup_bytes) L.wup = e->warena + e->canon_bytes + L.wup_off;
  }
  for (auto& n : e->norms) { n.g = (float*)(e->warena + n.g_off); n.b = (float*)(e->warena + n.b_off); }
  for (auto& t : e->tembs) {
    void* q = nullptr;
    if (dev_malloc(&q, (size_t)kMinVariantRows * t.cout_pad * 4) != 0) { g_create_err = "cannot allocate temb tables"; sdm_destroy(e); return SDM_ERR_NOMEM; }
    t.table = (float*)q;
    dev_memset(q, 0, (size_t)kMinVariantRows * t.cout_pad * 4, e->stream);
  }
  e->variant_cap = kMinVariantRows;
  dev_sync(e->stream);
  *out = e;
  return SDM_OK;
}

void sdm_destroy(sdm_ctx* e) {
  if (e) dev_use(e->device);
  if (!e) return;
  dev_sync(e->stream);
  arena_release_aside(e);
  if (e->warena) dev_free(e->warena);
  if (e->arena) dev_free(e->arena);
  if (e->stage) dev_free(e->stage);
  load_ring_release(e);
  if (e->io_in) dev_free(e->io_in);
  if (e->io_out) dev_free(e->io_out);
  if (e->d_bias_sel) dev_free(e->d_bias_sel);
  for (auto& t : e->tembs) if (t.table) dev_free(t.table);
#ifndef SDM_EMU
  if (e->ev0) (void)hipEventDestroy(e->ev0);
  if (e->ev1) (void)hipEventDestroy(e->ev1);
  if (e->ev_in) (void)hipEventDestroy(e->ev_in);
  if (e->ev_out) (void)hipEventDestroy(e->ev_out);
  if (e->own_stream) (void)hipStreamDestroy((hipStream_t)e->stream);
#endif
  delete e;
}

const char* sdm_last_error(sdm_ctx* e) { return e ? e->err.c_str() : g_create_err.c_str(); }

static float to_f32(const void* p, int dtype, size_t i) {
  if (dtype == SDM_F32) return ((const float*)p)[i];
  if (dtype == SDM_F16) return (float)((const half_t*)p)[i];
  uint32_t u = (uint32_t)((const uint16_t*)p)[i] << 16;   // bf16
  float f; memcpy(&f, &u, 4); return f;
}

// The one pack path of a layer's canonical tensors: fp32 OIHW / [O][I] weights (device) -> K16 w (+ w_lo of a split-precision layer), pre-scaled by
// w_scale * 2^w_exp, at input / output channel offsets ci_off / co_off of the layer; fp32 bias [n] -> b at co_off.
static void pack_layer_weight(sdm_ctx* e, const ConvL& L, const float* src, int O, int I, int ci_off, int co_off, float w_scale) {
  const size_t total = L.w_bytes() / 2;
  SDM_LAUNCH(pack_conv_weight_kernel, dim3((unsigned)std::min<size_t>((total + 255) / 256, 65535)), dim3(256), 0, e->stream, src, L.w, O, I, L.ntaps,
             L.Cin_pad, L.Cout_pad, ci_off, co_off, L.geglu, w_scale * ldexpf(1.0f, L.w_exp), L.w_lo);
}
// A weight the K16 format cannot hold: |w| * w_scale * 2^w_exp beyond fp16's largest finite value would be packed as inf and every output of the layer
// would be inf / nan with return code 0.  The load fails instead and names the tensor ("weights outside the split format").
static const float kK16Max = 65504.0f;
static int check_weight_range(sdm_ctx* e, const ConvL& L, const char* tensor, float amax, float w_scale) {
  const float packed = amax * fabsf(w_scale) * ldexpf(1.0f, L.w_exp);
  if (packed > kK16Max)
    SDM_FAIL(e, SDM_ERR_INVALID, "%s: max|w| = %g does not fit the packed fp16 weight format of layer %s (|w| * %g <= %g)", tensor, (double)amax, L.name.c_str(),
             (double)(fabsf(w_scale) * ldexpf(1.0f, L.w_exp)), (double)kK16Max);
  return 0;
}
static void pack_layer_bias(sdm_ctx* e, const ConvL& L, const float* src, int n, int co_off) {
  SDM_LAUNCH(pack_bias_kernel, dim3(sdm_cdiv(L.Cout_pad, 256)), dim3(256), 0, e->stream, src, L.b, n, L.Cout_pad, co_off, L.geglu);
}

int sdm_load_tensor(sdm_ctx* e, const char* name, int dtype, int ndim, const int64_t* shape, const void* host_ptr) {
  if (e) dev_use(e->device);
  if (!e || !name || !host_ptr) return SDM_ERR_INVALID;
  std::string key(name);
  // legacy VAE attention names
  static const char* legacy[4][2] = {{".query.", ".to_q."}, {".key.", ".to_k."}, {".value.", ".to_v."}, {".proj_attn.", ".to_out.0."}};
  if (key.find("mid_block.attentions.0") != std::string::npos)
    for (auto& l : legacy) { size_t pos = key.find(l[0]); if (pos != std::string::npos) key.replace(pos, strlen(l[0]), l[1]); }
  auto it = e->slots.find(key);
  if (it == e->slots.end()) { e->n_ignored++; return 0; }
  Slot& s = it->second;
  size_t n = 1, nexp = 1;
  for (int i = 0; i < ndim; ++i) n *= (size_t)shape[i];
  for (auto d : s.shape) nexp *= (size_t)d;
  bool ok = (n == nexp);
  if (ok && (s.kind == SLOT_CONV_W)) {
    ok = ndim >= 2 && shape[0] == s.shape[0] && shape[1] == s.shape[1];
  }
  if (!ok) SDM_FAIL(e, SDM_ERR_INVALID, "size mismatch for %s: checkpoint has %zu elements, model expects %zu", name, n, nexp);
  if (s.kind == SLOT_CONV_W) {
    float amax = 0.0f;
    for (size_t i = 0; i < n; ++i) amax = std::max(amax, fabsf(to_f32(host_ptr, dtype, i)));
    TRY(check_weight_range(e, e->convs[s.layer], name, amax, s.w_scale));
  }
  e->finalized = false;
  if (s.kind == SLOT_HOST) {
    float* dst = e->hostblob.data() + s.host_off;
    for (size_t i = 0; i < n; ++i) dst[i] = to_f32(host_ptr, dtype, i);
  } else {
    // convert to fp32 into a pinned staging slot, copy + pack asynchronously on the engine stream; the slot is reused only after
    // its event has fired (the ring keeps kLoadSlots tensors in flight)
    float* dsrc = nullptr;
#ifndef SDM_EMU
    sdm_ctx::LoadSlot& sl = e->load_ring[e->load_next];
    e->load_next = (e->load_next + 1) % sdm_ctx::kLoadSlots;
    if (sl.busy) { SDM_CHECK_DEV(e, (int)hipEventSynchronize(sl.done)); sl.busy = false; }
    if (sl.cap < n * 4) {
      if (sl.host) (void)hipHostFree(sl.host);
      if (sl.dev) dev_free(sl.dev);
      sl.host = sl.dev = nullptr; sl.cap = 0;
      const size_t cap = std::max(rupz(n * 4, (size_t)1 << 20), (size_t)8 << 20);
      if (hipHostMalloc(&sl.host, cap, hipHostMallocDefault) != hipSuccess || dev_malloc(&sl.dev, cap) != 0) SDM_FAIL(e, SDM_ERR_NOMEM, "weight staging alloc failed");
      sl.cap = cap;
      if (!sl.done) SDM_CHECK_DEV(e, (int)hipEventCreateWithFlags(&sl.done, hipEventDisableTiming));
    }
    float* hs = (float*)sl.host;
    if (dtype == SDM_F32) memcpy(hs, host_ptr, n * 4);
    else for (size_t i = 0; i < n; ++i) hs[i] = to_f32(host_ptr, dtype, i);
    SDM_CHECK_DEV(e, dev_memcpy_h2d(sl.dev, hs, n * 4, e->stream));
    dsrc = (float*)sl.dev;
#else
    if (ensure_buf(e, &e->stage, &e->stage_bytes, std::max(n * 4, (size_t)1 << 20)) != 0) return SDM_ERR_NOMEM;
    std::vector<float> tmp;
    const void* src = host_ptr;
    if (dtype != SDM_F32) { tmp.resize(n); for (size_t i = 0; i < n; ++i) tmp[i] = to_f32(host_ptr, dtype, i); src = tmp.data(); }
    SDM_CHECK_DEV(e, dev_memcpy_h2d(e->stage, src, n * 4, e->stream));
    dsrc = (float*)e->stage;
#endif
    if (s.host_too) {
      float* dst = e->hostblob.data() + s.host_off;
      for (size_t i = 0; i < n; ++i) dst[i] = to_f32(host_ptr, dtype, i);
    }
    if (s.kind == SLOT_CONV_W) {
      pack_layer_weight(e, e->convs[s.layer], dsrc, (int)s.shape[0], (int)s.shape[1], s.ci_off, s.co_off, s.w_scale);
    } else if (s.kind == SLOT_CONV_B) {
      pack_layer_bias(e, e->convs[s.layer], dsrc, (int)s.shape[0], s.co_off);
    } else {
      NormL& nn = e->norms[s.layer];
      SDM_CHECK_DEV(e, dev_memcpy_d2d(s.kind == SLOT_NORM_G ? nn.g : nn.b, dsrc, n * 4, e->stream));
    }
#ifndef SDM_EMU
    SDM_CHECK_DEV(e, (int)hipEventRecord(sl.done, (hipStream_t)e->stream));
    sl.busy = true;
#else
    SDM_CHECK_DEV(e, dev_sync(e->stream));
#endif
  }
  if (!s.loaded) { s.loaded = true; e->n_loaded++; }
  return 1;
}

// Exact fold of aux_conv_in into every cross-attention K|V projection; fp64 accumulation on the host.
//   kv_folded: K = P.Ak + 1.bk^T, V = P.Av + 1.bv^T with P the [Lk][36] patch matrix of the trimap latent (j = ci*9 + tap), Ak[j][o] = wf[o][j] = W_k . W_aux.
// One step further (the shared-operand form, option cross_shared): per head h the logits are Q_h K_h^T = (Q_h Ak_h^T) P^T + (Q_h bk_h) 1^T, whose second
// term is constant along the keys of a row and cancels in the softmax, exactly; and softmax(S_h) V_h = (softmax(S_h) P) Av_h + bv_h^T because the rows of a
// softmax sum to 1.  So the attention core can run on K = P, V^T = P^T (36 columns padded to the head dim 64) - the SAME operand for every head of every block,
// built once per forward (cross_patch_planes_kernel) - between two Linears of unchanged shape:
//   q_shared   [h*64 + j][c] = s . sum_d wf_k[h*64 + d][j] . Wq[h*64 + d][c]   (j < 36, else 0; s = the logit scale that w_scale folds into to_q; no bias)
//   out_shared [c][h*64 + j] = sum_d Wo[c][h*64 + d] . wf_v[h*64 + d][j]       (j < 36, else 0),  bias b_o[c] + sum_{h,d} Wo[c][h*64 + d] . bv[h*64 + d]
struct CrossFold { std::vector<float> wf, bf, wq, wo, bo; };
static void fold_cross_block(const sdm_ctx* e, const TfB& t, const std::vector<double>& wa, const std::vector<double>& ba, CrossFold& f) {
  const int ctx = e->cfg.cross_attention_dim, C = t.C;
  const float* H = e->hostblob.data();
  std::vector<double> wfd((size_t)2 * C * 36), bfd((size_t)2 * C);
  for (int o = 0; o < 2 * C; ++o) {
    const float* wrow = H + (o < C ? t.k_hoff + (size_t)o * ctx : t.v_hoff + (size_t)(o - C) * ctx);
    double b = 0.0;
    for (int m = 0; m < ctx; ++m) b += (double)wrow[m] * ba[m];
    bfd[o] = b;                                                  // W_k . b_aux   (to_k / to_v have no bias of their own)
    for (int j = 0; j < 36; ++j) {                               // j = ci*9 + tap (OIHW order of aux_conv_in.weight)
      const double* wj = wa.data() + (size_t)j * ctx;
      double acc = 0.0;
      for (int m = 0; m < ctx; ++m) acc += (double)wrow[m] * wj[m];
      wfd[(size_t)o * 36 + j] = acc;
    }
  }
  f.wf.resize(wfd.size()); f.bf.resize(bfd.size());
  for (size_t i = 0; i < wfd.size(); ++i) f.wf[i] = (float)wfd[i];
  for (size_t i = 0; i < bfd.size(); ++i) f.bf[i] = (float)bfd[i];
  const float* Wq = H + t.q_hoff;
  const float* Wo = H + t.o_hoff;
  const double s = (double)(0.125f * SDM_LOG2E);
  f.wq.assign((size_t)C * C, 0.f); f.wo.assign((size_t)C * C, 0.f); f.bo.assign((size_t)C, 0.f);
  std::vector<double> acc((size_t)C);
  for (int h = 0; h < t.heads; ++h)
    for (int j = 0; j < 36; ++j) {
      std::fill(acc.begin(), acc.end(), 0.0);
      for (int d = 0; d < 64; ++d) {
        const double a = wfd[(size_t)(h * 64 + d) * 36 + j];
        const float* row = Wq + (size_t)(h * 64 + d) * C;
        for (int c = 0; c < C; ++c) acc[c] += a * (double)row[c];
      }
      float* dst = f.wq.data() + (size_t)(h * 64 + j) * C;
      for (int c = 0; c < C; ++c) dst[c] = (float)(s * acc[c]);
    }
  for (int c = 0; c < C; ++c) {
    const float* row = Wo + (size_t)c * C;
    double b = (double)H[t.ob_hoff + c];
    for (int hd = 0; hd < C; ++hd) b += (double)row[hd] * bfd[(size_t)C + hd];
    f.bo[c] = (float)b;
    for (int h = 0; h < t.heads; ++h) {
      double a36[36] = {0.0};
      for (int d = 0; d < 64; ++d) {
        const double w = (double)row[h * 64 + d];
        const double* v = wfd.data() + (size_t)(C + h * 64 + d) * 36;
        for (int j = 0; j < 36; ++j) a36[j] += w * v[j];
      }
      for (int j = 0; j < 36; ++j) f.wo[(size_t)c * C + h * 64 + j] = (float)a36[j];
    }
  }
}
static int upload_folded(sdm_ctx* e, ConvL& L, const std::vector<float>& w, int O, int I, int ci_off, const std::vector<float>* bias) {
  if (ensure_buf(e, &e->stage, &e->stage_bytes, std::max(w.size() * 4, (size_t)1 << 20)) != 0) return SDM_ERR_NOMEM;
  float amax = 0.0f;
  for (float v : w) amax = std::max(amax, fabsf(v));
  TRY(check_weight_range(e, L, (L.name + " (folded cross-attention weight)").c_str(), amax, 1.0f));
  SDM_CHECK_DEV(e, dev_memset(L.w, 0, L.w_bytes(), e->stream));
  if (L.w_lo) SDM_CHECK_DEV(e, dev_memset(L.w_lo, 0, L.w_bytes(), e->stream));
  SDM_CHECK_DEV(e, dev_memcpy_h2d(e->stage, w.data(), w.size() * 4, e->stream));
  pack_layer_weight(e, L, (const float*)e->stage, O, I, ci_off, 0, 1.0f);
  SDM_CHECK_DEV(e, dev_sync(e->stream));
  if (bias) {
    SDM_CHECK_DEV(e, dev_memcpy_h2d(e->stage, bias->data(), bias->size() * 4, e->stream));
    pack_layer_bias(e, L, (const float*)e->stage, O, 0);
    SDM_CHECK_DEV(e, dev_sync(e->stream));
  }
  return 0;
}
static int fold_cross_kv(sdm_ctx* e) {
  const sdm_config& c = e->cfg;
  const int ctx = c.cross_attention_dim;
  const float* H = e->hostblob.data();
  // Waux transposed to [36][ctx] so that the inner loop is contiguous
  std::vector<double> wa((size_t)36 * ctx), ba(ctx);
  for (int m = 0; m < ctx; ++m) {
    ba[m] = H[e->h_auxb + m];
    for (int j = 0; j < 36; ++j) wa[(size_t)j * ctx + m] = H[e->h_auxw + (size_t)m * 36 + j];
  }
  std::vector<const TfB*> blocks;
  for (auto& v : e->u_down_tf) for (auto& t : v) blocks.push_back(&t);
  blocks.push_back(&e->u_midtf);
  for (auto& v : e->u_up_tf) for (auto& t : v) blocks.push_back(&t);
  // the blocks are independent (about 1.3 G fp64 multiply-adds at the full architecture): spread over a few host threads, uploaded in order afterwards
  std::vector<CrossFold> folds(blocks.size());
  {
    const unsigned hw = std::thread::hardware_concurrency();
    const size_t nthr = std::max<size_t>(1, std::min<size_t>(std::min<size_t>(hw ? hw : 1, 8), blocks.size()));
    std::atomic<size_t> next{0};
    auto work = [&]() { for (size_t i; (i = next.fetch_add(1)) < blocks.size();) fold_cross_block(e, *blocks[i], wa, ba, folds[i]); };
    std::vector<std::thread> pool;
    for (size_t i = 1; i < nthr; ++i) pool.emplace_back(work);
    work();
    for (auto& th : pool) th.join();
  }
  for (size_t i = 0; i < blocks.size(); ++i) {
    const TfB* t = blocks[i];
    const int C = t->C;
    // kv_folded: uploaded as an OIHW [2C][4][3][3] tensor; the 4 latent channels sit at channels 4..7 of the 16-channel U-Net input
    TRY(upload_folded(e, e->convs[t->kv2], folds[i].wf, 2 * C, 4, 4, &folds[i].bf));
    TRY(upload_folded(e, e->convs[t->q2s], folds[i].wq, C, C, 0, nullptr));
    TRY(upload_folded(e, e->convs[t->o2s], folds[i].wo, C, C, 0, &folds[i].bo));
    folds[i] = CrossFold();
  }
  return 0;
}

// Derived weight layouts (k_conv.h "derived weight layouts") of a set of layers from their canonical K16 tensors.  Two passes so that
// ONE host round trip serves every layer: the |max| of each fp8-residual layer (device reductions into a small table), then the
// layout kernels with the per-layer e4m3 scale 2^e8 = the largest power of two that keeps max|w| * 2^e8 <= 448.
static int derive_layers(sdm_ctx* e, std::vector<ConvL*>& layers) {
  std::vector<ConvL*> f8;
  for (ConvL* L : layers) if ((L->w_dma && L->f8) || L->w3) f8.push_back(L);
  const size_t n_own = f8.size();                                    // behind them: the layers with phase matrices, scaled by their largest summed weight
  for (ConvL* L : layers) if (L->wup) f8.push_back(L);
  if (!f8.empty()) {
    const size_t tb = rupz(f8.size() * 4, 256);
    if (ensure_buf(e, &e->stage, &e->stage_bytes, std::max(tb, (size_t)1 << 20)) != 0) return SDM_ERR_NOMEM;
    SDM_CHECK_DEV(e, dev_memset(e->stage, 0, tb, e->stream));
    for (size_t i = 0; i < f8.size(); ++i) {
      const size_t n = (size_t)f8[i]->Cin_pad * f8[i]->ntaps * f8[i]->Cout_pad;
      if (i >= n_own) {
        SDM_LAUNCH(up_phase_absmax_kernel, dim3(2048), dim3(256), 0, e->stream, (const half_t*)f8[i]->w, (const half_t*)f8[i]->w_lo, f8[i]->Cin_pad, f8[i]->Cout_pad,
                   (unsigned int*)e->stage + i);
        continue;
      }
      SDM_LAUNCH(absmax_f16_kernel, dim3((unsigned)std::min<size_t>((n + 255) / 256, 2048)), dim3(256), 0, e->stream, (const half_t*)f8[i]->w, n,
                 (unsigned int*)e->stage + i);
    }
    std::vector<float> mx(f8.size());
    SDM_CHECK_DEV(e, dev_memcpy_d2h(mx.data(), e->stage, f8.size() * 4, e->stream));
    SDM_CHECK_DEV(e, dev_sync(e->stream));
    for (size_t i = 0; i < f8.size(); ++i) {
      const float wmax = ldexpf(mx[i], -f8[i]->w_exp);            // K16 keeps w * 2^w_exp
      int ex = 8;
      if (wmax > 0.0f && std::isfinite(wmax)) {
        ex = (int)floorf(log2f(448.0f / wmax));
        while (ldexpf(wmax, ex) > 448.0f) --ex;                   // guard the rounding of log2f
        ex = std::max(-60, std::min(60, ex));
      }
      if (i >= n_own) f8[i]->up_exp = ex; else f8[i]->f8_exp = ex;
    }
  }
  for (ConvL* L : layers) {
    if (L->w3)
      SDM_LAUNCH(derive_gemm_w3_kernel<0>, dim3((unsigned)std::min<size_t>(((size_t)L->Cin_pad * L->Cout_pad / 4 + 255) / 256, 65535)), dim3(256), 0, e->stream,
                 (const half_t*)L->w, (const half_t*)L->w_lo, L->w3, L->Cin_pad, L->Cout_pad, ldexpf(1.0f, -L->w_exp), ldexpf(1.0f, L->f8_exp));
    if (L->wup)
      SDM_LAUNCH(derive_gemm_w3_kernel<1>, dim3((unsigned)std::min<size_t>(((size_t)L->Cin_pad * L->Cout_pad * 4 + 255) / 256, 65535)), dim3(256), 0, e->stream,
                 (const half_t*)L->w, (const half_t*)L->w_lo, L->wup, L->Cin_pad, L->Cout_pad, ldexpf(1.0f, -L->w_exp), ldexpf(1.0f, L->up_exp));
    if (!L->w_dma) continue;
    const size_t total = (size_t)L->Cin_pad * L->ntaps * L->Cout_pad;
    if (L->f8)
      SDM_LAUNCH(derive_conv_weight_f8_kernel, dim3((unsigned)std::min<size_t>((total / 4 + 255) / 256, 65535)), dim3(256), 0, e->stream,
                 (const half_t*)L->w, (const half_t*)L->w_lo, (unsigned char*)L->w_dma, L->Cin_pad, L->Cout_pad, L->ntaps, ldexpf(1.0f, -L->w_exp),
                 ldexpf(1.0f, L->f8_exp));
    else
      SDM_LAUNCH(derive_conv_weight_dma_kernel, dim3((unsigned)std::min<size_t>((total * (L->split ? 2 : 1) + 255) / 256, 65535)), dim3(256), 0, e->stream,
                 (const half_t*)L->w, (const half_t*)L->w_lo, L->w_dma, L->Cin_pad, L->Cout_pad, L->split ? 2 : 1);
  }
  SDM_CHECK_DEV(e, dev_sync(e->stream));
  return 0;
}

static void load_ring_release(sdm_ctx* e) {
#ifndef SDM_EMU
  for (auto& sl : e->load_ring) {
    if (sl.busy) { (void)hipEventSynchronize(sl.done); sl.busy = false; }
    if (sl.host) (void)hipHostFree(sl.host);
    if (sl.dev) dev_free(sl.dev);
    if (sl.done) (void)hipEventDestroy(sl.done);
    sl.host = sl.dev = nullptr; sl.cap = 0; sl.done = nullptr;
  }
#else
  (void)e;
#endif
}

int sdm_finalize_weights(sdm_ctx* e) {
  if (e) dev_use(e->device);
  if (!e) return SDM_ERR_INVALID;
  SDM_CHECK_DEV(e, dev_sync(e->stream));
  load_ring_release(e);          // the checkpoint is in: give the pinned / device staging ring back
  { int rc = fold_cross_kv(e); if (rc) return rc; }
  {   // the canonical K16 tensors are complete: build every derived layout from them
    std::vector<ConvL*> all;
    for (auto& L : e->convs) all.push_back(&L);
    int rc = derive_layers(e, all);
    if (rc) return rc;
  }
  e->missing.clear();
  for (auto& k : e->slot_order) if (!e->slots[k].loaded) e->missing.push_back(k);
  e->variants.clear();
  e->finalized = true;
  return SDM_OK;
}

int sdm_weight_stats(sdm_ctx* e, int64_t* n_loaded, int64_t* n_missing, int64_t* n_ignored) {
  if (!e) return SDM_ERR_INVALID;
  if (n_loaded) *n_loaded = e->n_loaded;
  if (n_missing) *n_missing = (int64_t)e->missing.size();
  if (n_ignored) *n_ignored = e->n_ignored;
  return SDM_OK;
}

const char* sdm_missing_key(sdm_ctx* e, int64_t i) {
  if (!e || i < 0 || i >= (int64_t)e->missing.size()) return nullptr;
  return e->missing[(size_t)i].c_str();
}

int64_t sdm_weight_blob_bytes(sdm_ctx* e) { return e ? (int64_t)e->canon_bytes : 0; }
int sdm_export_weight_blob(sdm_ctx* e, void* dst) {
  if (e) dev_use(e->device);
  if (!e || !dst) return SDM_ERR_INVALID;
  SDM_CHECK_DEV(e, dev_memcpy_d2d(dst, e->warena, e->canon_bytes, e->stream));
  SDM_CHECK_DEV(e, dev_sync(e->stream));
  return SDM_OK;
}
int sdm_import_weight_blob(sdm_ctx* e, const void* src) {
  if (e) dev_use(e->device);
  if (!e || !src) return SDM_ERR_INVALID;
  SDM_CHECK_DEV(e, dev_memcpy_d2d(e->warena, src, e->canon_bytes, e->stream));
  SDM_CHECK_DEV(e, dev_sync(e->stream));
  for (auto& kv : e->slots) if (kv.second.kind != SLOT_HOST && !kv.second.loaded) { kv.second.loaded = true; e->n_loaded++; }
  e->finalized = false;
  return SDM_OK;
}
int64_t sdm_host_blob_bytes(sdm_ctx* e) { return e ? (int64_t)(e->hostblob.size() * 4) : 0; }
int sdm_export_host_blob(sdm_ctx* e, void* dst) {
  if (!e || !dst) return SDM_ERR_INVALID;
  memcpy(dst, e->hostblob.data(), e->hostblob.size() * 4);
  return SDM_OK;
}
int sdm_import_host_blob(sdm_ctx* e, const void* src) {
  if (!e || !src) return SDM_ERR_INVALID;
  memcpy(e->hostblob.data(), src, e->hostblob.size() * 4);
  for (auto& kv : e->slots) if (kv.second.kind == SLOT_HOST && !kv.second.loaded) { kv.second.loaded = true; e->n_loaded++; }
  e->finalized = false;
  return SDM_OK;
}

int sdm_forward(sdm_ctx* e, const float* image, const float* trimap, int B, int S, const int32_t* is_trans, const float* coords, float* alpha,
                int ptr_kind, void* stream) {
  if (e) dev_use(e->device);
  if (!e || !image || !trimap || !alpha) return SDM_ERR_INVALID;
  return forward_impl(e, 0, image, trimap, B, S, S, S, is_trans, coords, 4, 0, true, alpha, ptr_kind, stream);
}

int sdm_forward_ex(sdm_ctx* e, const float* image, const float* aux, int B, int S, const int32_t* is_trans, const float* cond, int cond_dim,
                   int cond_kind, int use_attention_mask, float* alpha, int ptr_kind, void* stream) {
  if (e) dev_use(e->device);
  if (!e || !image || !aux || !alpha) return SDM_ERR_INVALID;
  if (cond_kind != SDM_COND_BOX && cond_kind != SDM_COND_POINTS) SDM_FAIL(e, SDM_ERR_INVALID, "unknown conditioning kind %d", cond_kind);
  return forward_impl(e, 0, image, aux, B, S, S, S, is_trans, cond, cond_dim, cond_kind, use_attention_mask != 0, alpha, ptr_kind, stream);
}

int sdm_forward_rect(sdm_ctx* e, const float* image, const float* aux, int B, int SH, int SW, const int32_t* is_trans, const float* cond,
                     int cond_dim, int cond_kind, int use_attention_mask, float* alpha, int ptr_kind, void* stream) {
  if (e) dev_use(e->device);
  if (!e || !image || !aux || !alpha) return SDM_ERR_INVALID;
  if (cond_kind != SDM_COND_BOX && cond_kind != SDM_COND_POINTS) SDM_FAIL(e, SDM_ERR_INVALID, "unknown conditioning kind %d", cond_kind);
  return forward_impl(e, 0, image, aux, B, SH, SW, 0, is_trans, cond, cond_dim, cond_kind, use_attention_mask != 0, alpha, ptr_kind, stream);
}

int sdm_apply_matte(sdm_ctx* e, const float* image, const float* trimap, int B, int H, int W, int S, int is_transparent, float* alpha,
                    int ptr_kind, void* stream) {
  if (e) dev_use(e->device);
  if (!e || !image || !trimap || !alpha) return SDM_ERR_INVALID;
  std::vector<int32_t> it((size_t)std::max(B, 1), is_transparent ? 1 : 0);
  return forward_impl(e, 1, image, trimap, B, H, W, S, it.data(), nullptr, 4, 0, true, alpha, ptr_kind, stream);
}

/* Give the activation arena and the I/O staging buffers back to the driver (weights stay resident).  The next forward
 * re-allocates what it needs. */
int sdm_release_memory(sdm_ctx* e) {
  if (e) dev_use(e->device);
  if (!e) return SDM_ERR_INVALID;
  SDM_CHECK_DEV(e, dev_sync(e->stream));
  if (e->arena) { dev_free(e->arena); e->arena = nullptr; e->arena_bytes = 0; }
  if (e->io_in) { dev_free(e->io_in); e->io_in = nullptr; e->io_in_bytes = 0; }
  if (e->io_out) { dev_free(e->io_out); e->io_out = nullptr; e->io_out_bytes = 0; }
  if (e->stage) { dev_free(e->stage); e->stage = nullptr; e->stage_bytes = 0; }
  return SDM_OK;
}
int sdm_set_option(const char* name, int value) {
  OptEntry* o = opt_find(name);
  if (!o) return SDM_ERR_INVALID;
  std::unique_lock<std::shared_mutex> g(g_opt_mu);      // waits for the forwards in flight on other host threads
  o->value = value;
  return SDM_OK;
}

int sdm_get_option(const char* name, int* value) {
  OptEntry* o = opt_find(name);
  if (!o || !value) return SDM_ERR_INVALID;
  *value = o->value;
  return SDM_OK;
}

void sdm_reset_options(void) {
  std::unique_lock<std::shared_mutex> g(g_opt_mu);
  for (auto& o : g_opts) o.value = o.def;
}

const char* sdm_option_name(int i) {
  return (i >= 0 && i < (int)(sizeof(g_opts) / sizeof(g_opts[0]))) ? g_opts[i].name : nullptr;
}

const char* sdm_option_help(int i) {
  return (i >= 0 && i < (int)(sizeof(g_opts) / sizeof(g_opts[0]))) ? g_opts[i].what : nullptr;
}

int sdm_kernel_counts(char* buf, int cap) {
  std::string out;
  std::lock_guard<std::mutex> g(g_count_mu);
  for (auto& kv : g_kernel_counts) { out += kv.first; out += "="; out += std::to_string(kv.second); out += ";"; }
  if (buf && cap > 0) { const int n = (int)out.size() < cap - 1 ? (int)out.size() : cap - 1; memcpy(buf, out.data(), (size_t)n); buf[n] = 0; }
  return (int)out.size();
}

void sdm_kernel_counts_reset(void) { std::lock_guard<std::mutex> g(g_count_mu); g_kernel_counts.clear(); }

int64_t sdm_weight_bytes(sdm_ctx* e) { return e ? (int64_t)e->warena_bytes : 0; }

int64_t sdm_resident_bytes(sdm_ctx* e) {
  return e ? (int64_t)(e->warena_bytes + e->arena_bytes + e->io_in_bytes + e->io_out_bytes + e->stage_bytes) : 0;
}

int sdm_apply_matte_node(sdm_ctx* e, const float* image, const float* trimap, int B, int H, int W, int trimap_h, int trimap_w, int S,
                         int is_transparent, int output_mode, int mask_refine, double trimap_constraint, float* alpha, float* matted, int ptr_kind,
                         void* stream) {
  if (e) dev_use(e->device);
  if (!e || !image || !trimap || !alpha || !matted) return SDM_ERR_INVALID;
  if (output_mode < 0 || output_mode > 2) SDM_FAIL(e, SDM_ERR_INVALID, "unknown output mode %d", output_mode);
  if (trimap_h <= 0 || trimap_w <= 0) SDM_FAIL(e, SDM_ERR_INVALID, "bad trimap size %dx%d", trimap_h, trimap_w);
  // the reference indexes the (H, W) alpha with the trimap only for mask_refine and matted_rgb (sdmatte_nodes.py:365-380,390-394):
  // only those need equal sizes
  if ((trimap_h != H || trimap_w != W) && (mask_refine || output_mode == 2))
    SDM_FAIL(e, SDM_ERR_INVALID, "trimap %dx%d does not match the image %dx%d (needed by mask_refine / matted_rgb)", trimap_h, trimap_w, H, W);
  std::vector<int32_t> it((size_t)std::max(B, 1), is_transparent ? 1 : 0);
  NodeTail tail; tail.output_mode = output_mode; tail.mask_refine = mask_refine ? 1 : 0; tail.c = trimap_constraint; tail.matted = matted;
  tail.TH = trimap_h; tail.TW = trimap_w;
  return forward_impl(e, 1, image, trimap, B, H, W, S, it.data(), nullptr, 4, 0, true, alpha, ptr_kind, stream, &tail);
}

int sdm_apply_matte_mask(sdm_ctx* e, const float* image, const float* mask, int B, int H, int W, int mask_h, int mask_w, int S, int is_transparent,
                         float threshold, int erode_px, int dilate_px, int output_mode, int mask_refine, double trimap_constraint, float* alpha,
                         float* matted, float* trimap_out, int ptr_kind, void* stream) {
  if (e) dev_use(e->device);
  if (!e || !image || !mask || !alpha || !matted) return SDM_ERR_INVALID;
  if (output_mode < 0 || output_mode > 2) SDM_FAIL(e, SDM_ERR_INVALID, "unknown output mode %d", output_mode);
  if (mask_h <= 0 || mask_w <= 0) SDM_FAIL(e, SDM_ERR_INVALID, "bad mask size %dx%d", mask_h, mask_w);
  // the size rule of sdm_apply_matte_node: the trimap made from the mask has the mask's size
  if ((mask_h != H || mask_w != W) && (mask_refine || output_mode == 2))
    SDM_FAIL(e, SDM_ERR_INVALID, "mask %dx%d does not match the image %dx%d (needed by mask_refine / matted_rgb)", mask_h, mask_w, H, W);
  TRY(trimap_check(e, std::max(B, 1), mask_h, mask_w, erode_px, dilate_px));
  std::vector<int32_t> it((size_t)std::max(B, 1), is_transparent ? 1 : 0);
  NodeTail tail; tail.output_mode = output_mode; tail.mask_refine = mask_refine ? 1 : 0; tail.c = trimap_constraint; tail.matted = matted;
  tail.TH = mask_h; tail.TW = mask_w;
  tail.from_mask = true; tail.threshold = threshold; tail.erode_px = erode_px; tail.dilate_px = dilate_px; tail.trimap_out = trimap_out;
  return forward_impl(e, 1, image, mask, B, H, W, S, it.data(), nullptr, 4, 0, true, alpha, ptr_kind, stream, &tail);
}

/* sdm_apply_matte_node / sdm_apply_matte_mask on the box of the trimap (k_roi.h): the box is an arena tensor of both passes and the model's input is
 * S x S whatever the box is, so the sizing pass never sees a data-dependent size. */
int sdm_apply_matte_roi(sdm_ctx* e, const float* image, const float* aux, int B, int H, int W, int S, int is_transparent, int aux_is_mask, float threshold,
                        int erode_px, int dilate_px, float roi_threshold, int margin_px, int margin_pct, int square, int output_mode, int mask_refine,
                        double trimap_constraint, float* alpha, float* matted, float* trimap_out, int32_t* roi_out, int ptr_kind, void* stream) {
  if (e) dev_use(e->device);
  if (!e || !image || !aux || !alpha || !matted) return SDM_ERR_INVALID;
  if (output_mode < 0 || output_mode > 2) SDM_FAIL(e, SDM_ERR_INVALID, "unknown output mode %d", output_mode);
  if (aux_is_mask != 0 && aux_is_mask != 1) SDM_FAIL(e, SDM_ERR_INVALID, "apply matte roi: aux_is_mask = %d must be 0 or 1", aux_is_mask);
  if (!aux_is_mask && trimap_out) SDM_FAIL(e, SDM_ERR_INVALID, "apply matte roi: trimap_out is written only with aux_is_mask = 1");
  TRY(roi_check(e, "apply matte roi", B, H, W, roi_threshold, margin_px, margin_pct, square));
  if (aux_is_mask) TRY(trimap_check(e, B, H, W, erode_px, dilate_px));
  std::vector<int32_t> it((size_t)B, is_transparent ? 1 : 0);
  NodeTail tail; tail.output_mode = output_mode; tail.mask_refine = mask_refine ? 1 : 0; tail.c = trimap_constraint; tail.matted = matted;
  tail.TH = H; tail.TW = W;
  if (aux_is_mask) { tail.from_mask = true; tail.threshold = threshold; tail.erode_px = erode_px; tail.dilate_px = dilate_px; tail.trimap_out = trimap_out; }
  tail.roi = true; tail.roi_threshold = roi_threshold; tail.margin_px = margin_px; tail.margin_pct = margin_pct; tail.square = square; tail.roi_out = roi_out;
  return forward_impl(e, 1, image, aux, B, H, W, S, it.data(), nullptr, 4, 0, true, alpha, ptr_kind, stream, &tail);
}

/* The box on its own (k_roi.h).  The raw extrema live in the activation arena.  Three launches, whatever the arguments. */
int sdm_subject_roi(sdm_ctx* e, const float* plane, int B, int H, int W, float roi_threshold, int margin_px, int margin_pct, int square, int32_t* roi,
                    int ptr_kind, void* stream_arg) {
  if (e) dev_use(e->device);
  if (!e || !plane || !roi) return SDM_ERR_INVALID;
  TRY(roi_check(e, "subject roi", B, H, W, roi_threshold, margin_px, margin_pct, square));
  IoSpan in[] = {{(void*)plane, (size_t)B * H * W * 4}}, out[] = {{roi, (size_t)B * 16}};
  return product_call(e, ptr_kind, stream_arg, in, out, [&]() -> int {
    T raw = talloc(e, B, 1, 1, 4, 1);
    if (!e->dry) op_roi_box(e, (const float*)in[0].p, B, H, W, roi_threshold, margin_px, margin_pct, square, (int*)raw.p, (int*)out[0].p);
    tfree(e, raw);
    return 0;
  });
}

/* Trimap from a mask on its own (k_trimap.h).  The distance plane lives in the activation arena. */
int sdm_make_trimap(sdm_ctx* e, const float* mask, int B, int H, int W, float threshold, int erode_px, int dilate_px, float* trimap, int ptr_kind,
                    void* stream_arg) {
  if (e) dev_use(e->device);
  if (!e || !mask || !trimap) return SDM_ERR_INVALID;
  TRY(trimap_check(e, B, H, W, erode_px, dilate_px));
  const size_t bytes = (size_t)B * H * W * 4;
  IoSpan in[] = {{(void*)mask, bytes}}, out[] = {{trimap, bytes}};
  return product_call(e, ptr_kind, stream_arg, in, out, [&]() -> int {
    T dist = talloc(e, B, H, W, 1, 0);
    if (!e->dry) op_trimap(e, (const float*)in[0].p, B, H, W, threshold, erode_px, dilate_px, (short*)dist.p, (float*)out[0].p);
    tfree(e, dist);
    return 0;
  });
}

// ------------------------------------------------------------------------------------------------
// foreground / background colours from image + alpha (k_foreground.h)
// ------------------------------------------------------------------------------------------------
struct FgLevel { int h, w; };

// the levels from (H, W) down to the largest small one (the last entry): everything in front of it is a launch of fg_level_kernel
static std::vector<FgLevel> fg_large_levels(int H, int W) {
  std::vector<FgLevel> lv;
  int h = H, w = W;
  while (std::max(h, w) > SDM_FG_SMALL) { lv.push_back({h, w}); h = (h + 1) / 2; w = (w + 1) / 2; }
  lv.push_back({h, w});
  return lv;
}

/* The level planes live in the activation arena. */
int sdm_estimate_foreground(sdm_ctx* e, const float* image, const float* alpha, int B, int H, int W, float regularization, float gradient_weight,
                            int n_small_iters, int n_big_iters, float* fg, int fg_channels, float* bg, int ptr_kind, void* stream_arg) {
  if (e) dev_use(e->device);
  if (!e || !image || !alpha || !fg) return SDM_ERR_INVALID;
  if (B <= 0 || H < 1 || W < 1) SDM_FAIL(e, SDM_ERR_INVALID, "estimate foreground: bad image size %dx%dx%d", B, H, W);
  if (H > SDM_FG_MAX_SIDE || W > SDM_FG_MAX_SIDE || (double)B * H * W > (double)SDM_FG_MAX_PIXELS)
    SDM_FAIL(e, SDM_ERR_INVALID, "estimate foreground: %dx%dx%d is too large (sides up to %d, %d pixels in all)", B, H, W, SDM_FG_MAX_SIDE, SDM_FG_MAX_PIXELS);
  if (!(regularization > 0.0f) || !std::isfinite(regularization))
    SDM_FAIL(e, SDM_ERR_INVALID, "estimate foreground: regularization = %g must be a finite number above 0", (double)regularization);
  if (!(gradient_weight >= 0.0f) || !std::isfinite(gradient_weight))
    SDM_FAIL(e, SDM_ERR_INVALID, "estimate foreground: gradient_weight = %g must be a finite number, 0 or above", (double)gradient_weight);
  if (n_small_iters < 1 || n_small_iters > SDM_FG_MAX_SMALL_ITERS)
    SDM_FAIL(e, SDM_ERR_INVALID, "estimate foreground: n_small_iters = %d outside 1 .. %d", n_small_iters, SDM_FG_MAX_SMALL_ITERS);
  if (n_big_iters < 1 || n_big_iters > SDM_FG_MAX_BIG_ITERS)
    SDM_FAIL(e, SDM_ERR_INVALID, "estimate foreground: n_big_iters = %d outside 1 .. %d", n_big_iters, SDM_FG_MAX_BIG_ITERS);
  if (fg_channels != 3 && fg_channels != 4) SDM_FAIL(e, SDM_ERR_INVALID, "estimate foreground: fg_channels = %d, must be 3 or 4", fg_channels);
  const size_t px = (size_t)B * H * W;
  IoSpan in[] = {{(void*)image, px * 12}, {(void*)alpha, px * 4}};
  IoSpan out[] = {{fg, px * 4 * fg_channels}, {bg, bg ? px * 12 : 0}};
  const std::vector<FgLevel> lv = fg_large_levels(H, W);
  const int nl = (int)lv.size();
  const int tw = fg_tile_w(n_big_iters), th = fg_tile_h(n_big_iters);
  return product_call(e, ptr_kind, stream_arg, in, out, [&]() -> int {
    const float* d_img = (const float*)in[0].p; const float* d_alpha = (const float*)in[1].p;
    float* d_fg = (float*)out[0].p; float* d_bg = (float*)out[1].p;
    // one plane of 8 floats per pixel for every level below the top one, the largest small level included: planes[i] belongs to lv[i]
    std::vector<T> planes((size_t)nl);
    for (int i = 1; i < nl; ++i) planes[i] = talloc(e, B, lv[i].h, lv[i].w, 8, 1);
    if (!e->dry) {
      const FgLevel s = lv[nl - 1];
      // the largest small level gathers 16 bytes per pixel and stores its result; the levels below it add about a third of its gathers
      prof_begin(e, "fg_small", 0, (double)B * s.h * s.w * (16 + (nl == 1 ? 4 * fg_channels + (bg ? 12 : 0) : 32)) * 4.0 / 3.0);
      count_kernel("fg_small");
      SDM_LAUNCH(fg_small_kernel, dim3((unsigned)B), dim3(SDM_FG_SMALL_PX), 0, e->stream, d_img, d_alpha, B, H, W, s.h, s.w, regularization, gradient_weight,
                 n_small_iters, (float*)planes[nl - 1].p, d_fg, fg_channels, d_bg);
      prof_end(e);
      for (int i = nl - 2; i >= 0; --i) {
        const double lpx = (double)B * lv[i].h * lv[i].w;
        // per pixel of the level: image 12 + alpha 4 + a quarter of a 32-byte pixel of the previous level, and the stores
        prof_begin(e, "fg_level", 0, lpx * (24 + (i == 0 ? 4 * fg_channels + (bg ? 12 : 0) : 32)));
        count_kernel("fg_level");
        SDM_LAUNCH(fg_level_kernel, dim3((unsigned)(B * sdm_cdiv(lv[i].h, th) * sdm_cdiv(lv[i].w, tw))), dim3(256), 0, e->stream, d_img, d_alpha, B, H, W,
                   lv[i].h, lv[i].w, (const float*)planes[i + 1].p, regularization, gradient_weight, n_big_iters, (float*)planes[i].p, d_fg, fg_channels, d_bg);
        prof_end(e);
      }
    }
    for (int i = nl - 1; i >= 1; --i) tfree(e, planes[i]);
    return 0;
  });
}

// ------------------------------------------------------------------------------------------------
// alpha refinement at full resolution: the subsampled colour guided filter (k_guided.h)
// ------------------------------------------------------------------------------------------------
/* The three coarse planes live in the activation arena.  Four launches, whatever the arguments. */
int sdm_refine_alpha_guided(sdm_ctx* e, const float* image, const float* alpha, int B, int H, int W, int subsample, int radius, float eps, float* out,
                            int ptr_kind, void* stream_arg) {
  if (e) dev_use(e->device);
  if (!e || !image || !alpha || !out) return SDM_ERR_INVALID;
  if (B <= 0 || H < 1 || W < 1) SDM_FAIL(e, SDM_ERR_INVALID, "refine alpha: bad image size %dx%dx%d", B, H, W);
  if (H > SDM_FG_MAX_SIDE || W > SDM_FG_MAX_SIDE || (double)B * H * W > (double)SDM_FG_MAX_PIXELS)
    SDM_FAIL(e, SDM_ERR_INVALID, "refine alpha: %dx%dx%d is too large (sides up to %d, %d pixels in all)", B, H, W, SDM_FG_MAX_SIDE, SDM_FG_MAX_PIXELS);
  if (subsample < 1 || subsample > SDM_GF_MAX_SUBSAMPLE)
    SDM_FAIL(e, SDM_ERR_INVALID, "refine alpha: subsample = %d outside 1 .. %d", subsample, SDM_GF_MAX_SUBSAMPLE);
  if (radius < 1 || radius > SDM_GF_MAX_RADIUS) SDM_FAIL(e, SDM_ERR_INVALID, "refine alpha: radius = %d outside 1 .. %d", radius, SDM_GF_MAX_RADIUS);
  if (!std::isfinite(eps) || !(eps >= 1e-6f) || !(eps <= 1.0f))
    SDM_FAIL(e, SDM_ERR_INVALID, "refine alpha: eps = %g must be a finite number in [1e-6, 1]", (double)eps);
  const size_t px = (size_t)B * H * W;
  IoSpan in[] = {{(void*)image, px * 12}, {(void*)alpha, px * 4}}, outs[] = {{out, px * 4}};
  const int s = subsample, h = sdm_cdiv(H, s), w = sdm_cdiv(W, s);
  const double cpx = (double)B * h * w;
  return product_call(e, ptr_kind, stream_arg, in, outs, [&]() -> int {
    const float* d_img = (const float*)in[0].p; const float* d_alpha = (const float*)in[1].p; float* d_out = (float*)outs[0].p;
    // runs of 4 pixels = 3 x 16 bytes of image: whole rows of them in the block-mean pass, the flat pixel index in the apply pass
    const bool mean_vec = W % 4 == 0 && (s == 1 || s == 2 || s % 4 == 0) && aligned16(d_img) && aligned16(d_alpha);
    const int apply_vec = aligned16(d_img) && aligned16(d_out) ? 1 : 0;
    // three planes of 4 floats per coarse pixel: (I', p'), (a, b), (abar, bbar)
    T coarse = talloc(e, B, h, w, 4, 1), ab = talloc(e, B, h, w, 4, 1), abar = talloc(e, B, h, w, 4, 1);
    if (!e->dry) {
      const int G = mean_vec && s < 4 ? 4 / s : 1;
      const dim3 mgrid((unsigned)sdm_cdiv(B * h * (w / G), 256)), blk(256);
      prof_begin(e, "gf_mean", 0, (double)px * 16 + cpx * 16);
      count_kernel("gf_mean");
      if (!mean_vec) SDM_LAUNCH((gf_mean_kernel<1, false>), mgrid, blk, 0, e->stream, d_img, d_alpha, B, H, W, s, h, w, (float*)coarse.p);
      else if (G == 4) SDM_LAUNCH((gf_mean_kernel<4, true>), mgrid, blk, 0, e->stream, d_img, d_alpha, B, H, W, s, h, w, (float*)coarse.p);
      else if (G == 2) SDM_LAUNCH((gf_mean_kernel<2, true>), mgrid, blk, 0, e->stream, d_img, d_alpha, B, H, W, s, h, w, (float*)coarse.p);
      else SDM_LAUNCH((gf_mean_kernel<1, true>), mgrid, blk, 0, e->stream, d_img, d_alpha, B, H, W, s, h, w, (float*)coarse.p);
      prof_end(e);
      const dim3 bgrid((unsigned)(B * sdm_cdiv(h, gf_tile_h(radius)) * sdm_cdiv(w, SDM_GF_TW)));
      prof_begin(e, "gf_fit", 0, cpx * 32);
      count_kernel("gf_fit");
      SDM_LAUNCH((gf_box_kernel<true>), bgrid, blk, 0, e->stream, (const float*)coarse.p, B, h, w, radius, eps, (float*)ab.p);
      prof_end(e);
      prof_begin(e, "gf_smooth", 0, cpx * 32);
      count_kernel("gf_smooth");
      SDM_LAUNCH((gf_box_kernel<false>), bgrid, blk, 0, e->stream, (const float*)ab.p, B, h, w, radius, eps, (float*)abar.p);
      prof_end(e);
      prof_begin(e, "gf_apply", 0, (double)px * 16 + cpx * 16);
      count_kernel("gf_apply");
      SDM_LAUNCH(gf_apply_kernel, dim3((unsigned)sdm_cdiv((int)((px + 3) / 4), 256)), blk, 0, e->stream, d_img, (const float*)abar.p, B, H, W, s, h, w,
                 apply_vec, d_out);
      prof_end(e);
    }
    tfree(e, abar); tfree(e, ab); tfree(e, coarse);
    return 0;
  });
}

// ------------------------------------------------------------------------------------------------
// temporal smoothing of the alpha, guided by the frames (k_temporal.h): the batch axis is time
// ------------------------------------------------------------------------------------------------
/* The argument limits that sdm_smooth_alpha_temporal and sdm_smooth_alpha_motion share. */
static int ts_check(sdm_ctx* e, int B, int H, int W, int clip_len, int radius, int patch, float color_tolerance, float strength, float max_change) {
  if (B <= 0 || H < 1 || W < 1) SDM_FAIL(e, SDM_ERR_INVALID, "smooth alpha: bad image size %dx%dx%d", B, H, W);
  if (H > SDM_FG_MAX_SIDE || W > SDM_FG_MAX_SIDE || (double)B * H * W > (double)SDM_FG_MAX_PIXELS)
    SDM_FAIL(e, SDM_ERR_INVALID, "smooth alpha: %dx%dx%d is too large (sides up to %d, %d pixels in all)", B, H, W, SDM_FG_MAX_SIDE, SDM_FG_MAX_PIXELS);
  if (clip_len < 0 || clip_len > B) SDM_FAIL(e, SDM_ERR_INVALID, "smooth alpha: clip_len = %d outside 0 .. B = %d", clip_len, B);
  if (radius < 1 || radius > SDM_TS_MAX_RADIUS) SDM_FAIL(e, SDM_ERR_INVALID, "smooth alpha: radius = %d outside 1 .. %d", radius, SDM_TS_MAX_RADIUS);
  if (patch < 0 || patch > SDM_TS_MAX_PATCH) SDM_FAIL(e, SDM_ERR_INVALID, "smooth alpha: patch = %d outside 0 .. %d", patch, SDM_TS_MAX_PATCH);
  if (!std::isfinite(color_tolerance) || !(color_tolerance >= 1.0f / 1024.0f) || !(color_tolerance <= 1.0f))
    SDM_FAIL(e, SDM_ERR_INVALID, "smooth alpha: color_tolerance = %g must be a finite number in [1/1024, 1]", (double)color_tolerance);
  if (!std::isfinite(strength) || !(strength >= 0.0f) || !(strength <= 1.0f))
    SDM_FAIL(e, SDM_ERR_INVALID, "smooth alpha: strength = %g must be a finite number in [0, 1]", (double)strength);
  if (!std::isfinite(max_change) || !(max_change >= 0.0f) || !(max_change <= 1.0f))
    SDM_FAIL(e, SDM_ERR_INVALID, "smooth alpha: max_change = %g must be a finite number in [0, 1]", (double)max_change);
  return 0;
}

/* Nothing in the arena.  One launch, whatever the arguments. */
int sdm_smooth_alpha_temporal(sdm_ctx* e, const float* image, const float* alpha, int B, int H, int W, int clip_len, int radius, int patch,
                              float color_tolerance, float strength, float max_change, float* out, int ptr_kind, void* stream_arg) {
  if (e) dev_use(e->device);
  if (!e || !image || !alpha || !out) return SDM_ERR_INVALID;
  if (int rc = ts_check(e, B, H, W, clip_len, radius, patch, color_tolerance, strength, max_change)) return rc;
  const size_t px = (size_t)B * H * W;
  IoSpan in[] = {{(void*)image, px * 12}, {(void*)alpha, px * 4}}, outs[] = {{out, px * 4}};
  const int L = clip_len ? clip_len : B;
  const float tau2 = color_tolerance * color_tolerance;
  return product_call(e, ptr_kind, stream_arg, in, outs, [&]() -> int {
    const float* d_img = (const float*)in[0].p; const float* d_alpha = (const float*)in[1].p; float* d_out = (float*)outs[0].p;
    if (!e->dry) {
      const int vec = W % 4 == 0 && aligned16(d_img) && aligned16(d_alpha) && aligned16(d_out) ? 1 : 0;
      const dim3 grid((unsigned)(sdm_cdiv(B, L) * sdm_cdiv(H, ts_tile_h(patch)) * sdm_cdiv(W, SDM_TS_TW))), blk(256);
      prof_begin(e, "ts_smooth", 0, (double)px * 20);
      count_kernel("ts_smooth");
#define SDM_TS_CASE(R, P) \
  case (R) * 3 + (P): SDM_LAUNCH((ts_smooth_kernel<R, P>), grid, blk, 0, e->stream, d_img, d_alpha, B, H, W, L, tau2, strength, max_change, vec, d_out); break
      switch (radius * 3 + patch) {
        SDM_TS_CASE(1, 0); SDM_TS_CASE(1, 1); SDM_TS_CASE(1, 2); SDM_TS_CASE(2, 0); SDM_TS_CASE(2, 1); SDM_TS_CASE(2, 2);
        SDM_TS_CASE(3, 0); SDM_TS_CASE(3, 1); SDM_TS_CASE(3, 2); SDM_TS_CASE(4, 0); SDM_TS_CASE(4, 1); SDM_TS_CASE(4, 2);
      }
#undef SDM_TS_CASE
      prof_end(e);
    }
    return 0;
  });
}

/* The pixels of [lo - halo, lo + len + halo) that lie in [0, n), summed over the tiles lo = 0, len, 2 len, .. of n: what tsm_smooth_kernel's blocks fetch
 * along one axis. */
static double tsm_axis_px(int n, int len, int halo) {
  double s = 0;
  for (int lo = 0; lo < n; lo += len) s += std::min(n, lo + len + halo) - std::max(0, lo - halo);
  return s;
}

/* The same filter along a block-matched displacement (k_motion.h).  Nothing in the arena.  One launch for search >= 1; search == 0 IS the call above. */
int sdm_smooth_alpha_motion(sdm_ctx* e, const float* image, const float* alpha, int B, int H, int W, int clip_len, int radius, int patch, int search,
                            float color_tolerance, float motion_penalty, float strength, float max_change, float* out, int ptr_kind, void* stream_arg) {
  if (e) dev_use(e->device);
  if (!e || !image || !alpha || !out) return SDM_ERR_INVALID;
  if (search < 0 || search > SDM_TSM_MAX_SEARCH) SDM_FAIL(e, SDM_ERR_INVALID, "smooth alpha: search = %d outside 0 .. %d", search, SDM_TSM_MAX_SEARCH);
  if (search == 0) return sdm_smooth_alpha_temporal(e, image, alpha, B, H, W, clip_len, radius, patch, color_tolerance, strength, max_change, out, ptr_kind, stream_arg);
  if (int rc = ts_check(e, B, H, W, clip_len, radius, patch, color_tolerance, strength, max_change)) return rc;
  if (!std::isfinite(motion_penalty) || !(motion_penalty >= 0.0f) || !(motion_penalty <= 1.0f))
    SDM_FAIL(e, SDM_ERR_INVALID, "smooth alpha: motion_penalty = %g must be a finite number in [0, 1]", (double)motion_penalty);
  static_assert(SDM_TSM_S == SDM_TSM_MAX_SEARCH && SDM_TS_MAX_PATCH == 2, "k_motion.h sizes its LDS region for these");
  const size_t px = (size_t)B * H * W;
  IoSpan in[] = {{(void*)image, px * 12}, {(void*)alpha, px * 4}}, outs[] = {{out, px * 4}};
  const int L = clip_len ? clip_len : B;
  const float tau2 = color_tolerance * color_tolerance;
  const float pt = motion_penalty * tau2;
  return product_call(e, ptr_kind, stream_arg, in, outs, [&]() -> int {
    const float* d_img = (const float*)in[0].p; const float* d_alpha = (const float*)in[1].p; float* d_out = (float*)outs[0].p;
    if (!e->dry) {
      const int vec = W % 4 == 0 && aligned16(d_img) && aligned16(d_alpha) ? 1 : 0;
      const int tw = tsm_tile_w(patch);
      const dim3 grid((unsigned)(B * sdm_cdiv(H, SDM_TSM_TH) * sdm_cdiv(W, tw))), blk(256);
      // bytes: every block fetches its target region once and a larger region of each neighbour of its frame (16 bytes per pixel), and writes its tile
      double pairs = 0;
      for (int t = 0; t < B; ++t) pairs += std::min(t + radius, std::min(B, (t / L) * L + L) - 1) - std::max(t - radius, (t / L) * L);
      const double bytes = 16.0 * (B * tsm_axis_px(H, SDM_TSM_TH, patch) * tsm_axis_px(W, tw, patch) +
                                   pairs * tsm_axis_px(H, SDM_TSM_TH, patch + search) * tsm_axis_px(W, tw, patch + search)) + 4.0 * (double)px;
      prof_begin(e, "tsm_smooth", 0, bytes);
      count_kernel("tsm_smooth");
#define SDM_TSM_CASE(P) \
  case P: SDM_LAUNCH((tsm_smooth_kernel<P>), grid, blk, 0, e->stream, d_img, d_alpha, B, H, W, L, radius, search, tau2, pt, strength, max_change, vec, d_out); break
      switch (patch) { SDM_TSM_CASE(0); SDM_TSM_CASE(1); SDM_TSM_CASE(2); }
#undef SDM_TSM_CASE
      prof_end(e);
    }
    return 0;
  });
}

// ------------------------------------------------------------------------------------------------
// the subject over its own background out of focus (k_defocus.h)
// ------------------------------------------------------------------------------------------------
/* The prefix plane (16 bytes per pixel) lives in the activation arena.  Two launches, whatever the arguments. */
int sdm_defocus_background(sdm_ctx* e, const float* image, const float* alpha, const float* fg, const float* bg, int B, int H, int W, int radius_px,
                           float highlight_gain, float highlight_threshold, float* out, int ptr_kind, void* stream_arg) {
  if (e) dev_use(e->device);
  if (!e || !image || !alpha || !out) return SDM_ERR_INVALID;
  if (B <= 0 || H < 1 || W < 1) SDM_FAIL(e, SDM_ERR_INVALID, "defocus background: bad image size %dx%dx%d", B, H, W);
  if (H > SDM_FG_MAX_SIDE || W > SDM_FG_MAX_SIDE || (double)B * H * W > (double)SDM_FG_MAX_PIXELS)
    SDM_FAIL(e, SDM_ERR_INVALID, "defocus background: %dx%dx%d is too large (sides up to %d, %d pixels in all)", B, H, W, SDM_FG_MAX_SIDE, SDM_FG_MAX_PIXELS);
  if (radius_px < 1 || radius_px > SDM_DEFOCUS_MAX_RADIUS)
    SDM_FAIL(e, SDM_ERR_INVALID, "defocus background: radius_px = %d outside 1 .. %d", radius_px, SDM_DEFOCUS_MAX_RADIUS);
  if (!std::isfinite(highlight_gain) || !(highlight_gain >= 0.0f) || !(highlight_gain <= (float)SDM_DEFOCUS_MAX_GAIN))
    SDM_FAIL(e, SDM_ERR_INVALID, "defocus background: highlight_gain = %g must be a finite number in [0, %d]", (double)highlight_gain, SDM_DEFOCUS_MAX_GAIN);
  if (!std::isfinite(highlight_threshold) || !(highlight_threshold >= 0.0f) || !(highlight_threshold <= 1.0f))
    SDM_FAIL(e, SDM_ERR_INVALID, "defocus background: highlight_threshold = %g must be a finite number in [0, 1]", (double)highlight_threshold);
  static_assert(SDM_DOF_R == SDM_DEFOCUS_MAX_RADIUS && 2 * SDM_DOF_R + 1 < SDM_DOF_SEG && SDM_DOF_FLOOR == SDM_DEFOCUS_FLOOR, "k_defocus.h is sized for these");
  DofDisc disc;
  memset(&disc, 0, sizeof(disc));
  disc.r = radius_px;
  for (int dy = 0, h = radius_px; dy <= radius_px; ++dy) {      // the largest h with h h <= R R - dy dy, in integers
    while (h * h > radius_px * radius_px - dy * dy) --h;
    disc.hw[dy] = (unsigned char)h;
  }
  const size_t px = (size_t)B * H * W;
  // (an absent plane is an empty span behind a valid pointer: the staging copies 0 bytes of it)
  IoSpan in[] = {{(void*)image, px * 12}, {(void*)alpha, px * 4}, {(void*)(fg ? fg : image), fg ? px * 12 : 0}, {(void*)(bg ? bg : image), bg ? px * 12 : 0}};
  IoSpan outs[] = {{out, px * 12}};
  return product_call(e, ptr_kind, stream_arg, in, outs, [&]() -> int {
    const float* d_img = (const float*)in[0].p; const float* d_alpha = (const float*)in[1].p; float* d_out = (float*)outs[0].p;
    const float* d_F = fg ? (const float*)in[2].p : d_img; const float* d_C = bg ? (const float*)in[3].p : d_img;
    T plane = talloc(e, B, H, W, 4, 1);
    if (!e->dry) {
      const int vec = W % 4 == 0 && aligned16(d_C) && aligned16(d_alpha) ? 1 : 0;
      const long long units = (long long)B * H * sdm_cdiv(W, SDM_DOF_SEG);
      prof_begin(e, "dof_prefix", 0, (double)px * 32);
      count_kernel("dof_prefix");
      SDM_LAUNCH(dof_prefix_kernel, dim3((unsigned)((units + 3) / 4)), dim3(256), 0, e->stream, d_C, d_alpha, B, H, W, highlight_gain, highlight_threshold, vec,
                 (f32x4*)plane.p);
      prof_end(e);
      // bytes: every tile fetches its window of the prefix plane (rows and columns within radius_px of it, 16 bytes per pixel); the epilogue reads C, F
      // and the alpha and writes the result
      double win_px = 0;
      for (int y0 = 0; y0 < H; y0 += SDM_DOF_TH) {
        const double rows = std::min(H - 1, y0 + SDM_DOF_TH - 1 + radius_px) - std::max(0, y0 - radius_px) + 1;
        for (int x0 = 0; x0 < W; x0 += SDM_DOF_TW) win_px += rows * (std::min(W - 1, x0 + SDM_DOF_TW - 1 + radius_px) - std::max(0, x0 - radius_px - 1) + 1);
      }
      prof_begin(e, "dof_gather", 0, 16.0 * B * win_px + (double)px * (4 + 12 + (d_F != d_C ? 12 : 0) + 12));
      count_kernel("dof_gather");
      SDM_LAUNCH(dof_gather_kernel, dim3((unsigned)(B * sdm_cdiv(H, SDM_DOF_TH) * sdm_cdiv(W, SDM_DOF_TW))), dim3(256), 0, e->stream, (const f32x4*)plane.p, d_C, d_F,
                 d_alpha, B, H, W, disc, d_out);
      prof_end(e);
    }
    tfree(e, plane);
    return 0;
  });
}

// ------------------------------------------------------------------------------------------------
// the photo without its subject: push-pull fill (k_plate.h)
// ------------------------------------------------------------------------------------------------
/* The pyramid (levels 1 .. S, 16 bytes per pixel, about a third of a level-0 plane of that width) lives in the activation arena.  1 + 2 ceil(S / 3)
 * launches, S = the number of levels with max(h_l, w_l) > 32: a function of H and W only. */
int sdm_fill_background(sdm_ctx* e, const float* image, const float* alpha, const float* bg, const float* hole, int B, int H, int W, float alpha_cut,
                        float* out, int ptr_kind, void* stream_arg) {
  if (e) dev_use(e->device);
  if (!e || !image || !alpha || !out) return SDM_ERR_INVALID;
  if (B <= 0 || H < 1 || W < 1) SDM_FAIL(e, SDM_ERR_INVALID, "fill background: bad image size %dx%dx%d", B, H, W);
  if (H > SDM_FG_MAX_SIDE || W > SDM_FG_MAX_SIDE || (double)B * H * W > (double)SDM_FG_MAX_PIXELS)
    SDM_FAIL(e, SDM_ERR_INVALID, "fill background: %dx%dx%d is too large (sides up to %d, %d pixels in all)", B, H, W, SDM_FG_MAX_SIDE, SDM_FG_MAX_PIXELS);
  if (!std::isfinite(alpha_cut) || !(alpha_cut >= SDM_PLATE_MIN_CUT) || !(alpha_cut <= 1.0f))
    SDM_FAIL(e, SDM_ERR_INVALID, "fill background: alpha_cut = %g must be a finite number in [%g, 1]", (double)alpha_cut, (double)SDM_PLATE_MIN_CUT);
  static_assert(SDM_PLATE_SMALL_PX == SDM_PLATE_SMALL * SDM_PLATE_SMALL && SDM_PLATE_GROUP == 3 && SDM_PLATE_TW == 64 && SDM_PLATE_TH == 32,
                "k_plate.h is written for these");
  int S = 0;
  while (std::max(plate_dim(H, S), plate_dim(W, S)) > SDM_PLATE_SMALL) ++S;
  size_t off[17] = {0}, pyr_px = 0;                                     // off[l]: first pixel of level l's plane, l = 1 .. S (SDM_FG_MAX_SIDE = 2^15: S <= 10)
  for (int l = 1; l <= S; ++l) { off[l] = pyr_px; pyr_px += (size_t)B * plate_dim(H, l) * plate_dim(W, l); }
  const size_t px = (size_t)B * H * W;
  // (an absent plane is an empty span behind a valid pointer: the staging copies 0 bytes of it; with bg the image is not read)
  IoSpan in[] = {{(void*)image, bg ? 0 : px * 12}, {(void*)alpha, px * 4}, {(void*)(bg ? bg : image), bg ? px * 12 : 0},
                 {(void*)(hole ? hole : alpha), hole ? px * 4 : 0}};
  IoSpan outs[] = {{out, px * 12}};
  return product_call(e, ptr_kind, stream_arg, in, outs, [&]() -> int {
    const float* d_alpha = (const float*)in[1].p; float* d_out = (float*)outs[0].p;
    const float* d_C = bg ? (const float*)in[2].p : (const float*)in[0].p; const float* d_hole = hole ? (const float*)in[3].p : nullptr;
    T pyr;
    if (S > 0) pyr = talloc(e, 1, 1, (int)pyr_px, 4, 1);
    if (!e->dry) {
      PlateIn pin;
      pin.C = d_C; pin.alpha = d_alpha; pin.hole = d_hole; pin.cut = alpha_cut;
      pin.vec = W % 4 == 0 && aligned16(d_C) && aligned16(d_alpha) && (!d_hole || aligned16(d_hole)) && aligned16(d_out) ? 1 : 0;
      auto plane = [&](int l) -> f32x4* { return (l >= 1 && l <= S) ? (f32x4*)pyr.p + off[l] : nullptr; };
      auto lpx = [&](int l) -> double { return (double)B * plate_dim(H, l) * plate_dim(W, l); };
      const double in_bpp = 16.0 + (d_hole ? 4.0 : 0.0);
      auto tiles = [&](int l) -> unsigned { return (unsigned)(B * sdm_cdiv(plate_dim(H, l), SDM_PLATE_TH) * sdm_cdiv(plate_dim(W, l), SDM_PLATE_TW)); };
      for (int l = 0; l < S; l += SDM_PLATE_GROUP) {
        const int n = std::min(SDM_PLATE_GROUP, S - l);
        double bytes = lpx(l) * (l ? 16.0 : in_bpp);
        for (int k = 1; k <= n; ++k) bytes += 16.0 * lpx(l + k);
        prof_begin(e, "plate_pull", 0, bytes);
        count_kernel("plate_pull");
        SDM_LAUNCH(plate_pull_kernel, dim3(tiles(l)), dim3(256), 0, e->stream, pin, (const f32x4*)plane(l), B, H, W, l, n, plane(l + 1), plane(l + 2),
                   plane(l + 3));
        prof_end(e);
      }
      prof_begin(e, "plate_small", 0, S ? 32.0 * lpx(S) : (double)px * (in_bpp + 12.0));
      count_kernel("plate_small");
      SDM_LAUNCH(plate_small_kernel, dim3((unsigned)B), dim3(SDM_PLATE_SMALL_PX), 0, e->stream, pin, plane(S), B, H, W, S, d_out);
      prof_end(e);
      for (int top = S; top > 0;) {                                     // the first push takes what three do not divide
        const int n = top % SDM_PLATE_GROUP ? top % SDM_PLATE_GROUP : SDM_PLATE_GROUP, lf = top - n;
        // bytes: the tile's own level in and out; the levels above it with their halo (counted without it: a ring of one pixel)
        double bytes = lf ? 32.0 * lpx(lf) : (double)px * (in_bpp + 12.0);
        for (int k = 1; k <= n; ++k) bytes += 16.0 * lpx(lf + k);
        prof_begin(e, "plate_push", 0, bytes);
        count_kernel("plate_push");
        SDM_LAUNCH(plate_push_kernel, dim3(tiles(lf)), dim3(256), 0, e->stream, pin, (const f32x4*)plane(top), (const f32x4*)(n == 3 ? plane(lf + 2) : nullptr),
                   (const f32x4*)(n >= 2 ? plane(lf + 1) : nullptr), plane(lf), B, H, W, lf, n, d_out);
        prof_end(e);
        top = lf;
      }
    }
    if (S > 0) tfree(e, pyr);
    return 0;
  });
}

// ------------------------------------------------------------------------------------------------
// the cut-out in its new scene: colour match and light wrap (k_harmonize.h)
// ------------------------------------------------------------------------------------------------
/* The partial sums (14 floats per run of 4096 pixels), the map (12 floats per image) and, with the wrap, the row-blurred plane (16 bytes per pixel) live in
 * the activation arena.  hz_stats and hz_finalize run when the match is on, hz_rows when the wrap is on, hz_compose always. */
int sdm_harmonize(sdm_ctx* e, const float* fg, const float* alpha, const float* bg_image, int bg_batch, int B, int H, int W, float luma_strength,
                  float chroma_strength, float contrast_strength, float wrap_strength, float wrap_sigma, float* out, float* fg_out, float* map_out,
                  int ptr_kind, void* stream_arg) {
  if (e) dev_use(e->device);
  if (!e || !fg || !alpha || !bg_image || !out) return SDM_ERR_INVALID;
  if (B <= 0 || H < 1 || W < 1) SDM_FAIL(e, SDM_ERR_INVALID, "harmonize: bad image size %dx%dx%d", B, H, W);
  if (H > SDM_FG_MAX_SIDE || W > SDM_FG_MAX_SIDE || (double)B * H * W > (double)SDM_FG_MAX_PIXELS)
    SDM_FAIL(e, SDM_ERR_INVALID, "harmonize: %dx%dx%d is too large (sides up to %d, %d pixels in all)", B, H, W, SDM_FG_MAX_SIDE, SDM_FG_MAX_PIXELS);
  if (bg_batch != 1 && bg_batch != B) SDM_FAIL(e, SDM_ERR_INVALID, "harmonize: bg_batch = %d must be 1 or %d", bg_batch, B);
  const struct { const char* name; float v; } strengths[] = {{"luma_strength", luma_strength}, {"chroma_strength", chroma_strength},
                                                             {"contrast_strength", contrast_strength}, {"wrap_strength", wrap_strength}};
  for (const auto& s : strengths)
    if (!std::isfinite(s.v) || !(s.v >= 0.0f) || !(s.v <= 1.0f))
      SDM_FAIL(e, SDM_ERR_INVALID, "harmonize: %s = %g must be a finite number in [0, 1]", s.name, (double)s.v);
  const bool match = luma_strength > 0.0f || chroma_strength > 0.0f, wrap = wrap_strength > 0.0f;
  if (wrap && (!std::isfinite(wrap_sigma) || !(wrap_sigma > 0.0f) || !(wrap_sigma <= (float)SDM_HZ_MAX_WRAP_SIGMA)))
    SDM_FAIL(e, SDM_ERR_INVALID, "harmonize: wrap_sigma = %g must be a finite number in (0, %d]", (double)wrap_sigma, SDM_HZ_MAX_WRAP_SIGMA);
  static_assert(SDM_HZ_R == 3 * SDM_HZ_MAX_WRAP_SIGMA && SDM_HZ_R % 4 == 0 && SDM_HZ_RUN_PX == SDM_HZ_RUN, "k_harmonize.h is sized for these");
  HzBlur blur;
  memset(&blur, 0, sizeof(blur));
  if (wrap) {      // w_i = exp(-i^2 / (2 sigma^2)) / sum, in double, rounded to fp32 (as the shadow of sdm_compose_canvas)
    const double s = (double)wrap_sigma;
    blur.r = std::min(SDM_HZ_R, std::max(1, (int)std::ceil(3.0 * s)));
    double g[2 * SDM_HZ_R + 1], sum = 0.0;
    for (int k = 0; k <= 2 * blur.r; ++k) { const double i = (double)(k - blur.r); g[k] = std::exp(-(i * i) / (2.0 * s * s)); sum += g[k]; }
    for (int k = 0; k <= 2 * blur.r; ++k) blur.w[k] = (float)(g[k] / sum);
  }
  const HzParams prm = {luma_strength, chroma_strength, contrast_strength, wrap_strength};
  const size_t px = (size_t)B * H * W;
  const int runs = sdm_cdiv(H * W, SDM_HZ_RUN_PX);
  IoSpan in[] = {{(void*)fg, px * 12}, {(void*)alpha, px * 4}, {(void*)bg_image, (size_t)bg_batch * H * W * 12}};
  IoSpan outs[] = {{out, px * 12}, {fg_out, fg_out ? px * 12 : 0}, {map_out, map_out ? (size_t)B * 48 : 0}};
  return product_call(e, ptr_kind, stream_arg, in, outs, [&]() -> int {
    const float* d_fg = (const float*)in[0].p; const float* d_alpha = (const float*)in[1].p; const float* d_bg = (const float*)in[2].p;
    float* d_out = (float*)outs[0].p; float* d_fg_out = fg_out ? (float*)outs[1].p : nullptr; float* d_map_out = map_out ? (float*)outs[2].p : nullptr;
    T partials, map, tplane;
    if (match) { partials = talloc(e, B, runs, 1, SDM_HZ_NSUM, 1); map = talloc(e, B, 1, 1, 12, 1); }
    if (wrap) tplane = talloc(e, B, H, W, 4, 1);
    if (!e->dry) {
      const double bg_px = (double)bg_batch * H * W;
      if (match) {
        const int vec = (H * W) % 4 == 0 && aligned16(d_fg) && aligned16(d_alpha) && aligned16(d_bg) ? 1 : 0;
        prof_begin(e, "hz_stats", 0, (double)px * 16 + bg_px * 12 + (double)B * runs * 56);
        count_kernel("hz_stats");
        SDM_LAUNCH(hz_stats_kernel, dim3((unsigned)(B * runs)), dim3(256), 0, e->stream, d_fg, d_alpha, d_bg, bg_batch, B, H, W, vec, (float*)partials.p);
        prof_end(e);
        prof_begin(e, "hz_finalize", 0, (double)B * runs * 56);
        count_kernel("hz_finalize");
        SDM_LAUNCH(hz_finalize_kernel, dim3((unsigned)B), dim3(64), 0, e->stream, (const float*)partials.p, B, runs, prm, (double)SDM_HZ_VAR_FLOOR,
                   (double)SDM_HZ_MAX_GAIN, (double)SDM_HZ_MIN_WEIGHT, (float*)map.p, d_map_out);
        prof_end(e);
      }
      if (wrap) {
        const int vec = W % 4 == 0 && aligned16(d_alpha) && aligned16(d_bg) ? 1 : 0;
        const long long units = (long long)B * H * sdm_cdiv(W, SDM_HZ_SEG);
        prof_begin(e, "hz_rows", 0, (double)px * (4 + 12 + 16));
        count_kernel("hz_rows");
        SDM_LAUNCH(hz_rows_kernel, dim3((unsigned)((units + 3) / 4)), dim3(256), 0, e->stream, d_alpha, d_bg, bg_batch, B, H, W, blur, vec, (f32x4*)tplane.p);
        prof_end(e);
      }
      // bytes: fg, alpha, bg and the results once; every tile fetches the rows of T within r of it
      double win_rows = 0;
      if (wrap)
        for (int y0 = 0; y0 < H; y0 += SDM_HZ_TH) win_rows += std::min(H - 1, y0 + SDM_HZ_TH - 1 + blur.r) - std::max(0, y0 - blur.r) + 1;
      prof_begin(e, "hz_compose", 0, (double)px * (12 + 4 + 12 + 12 + (d_fg_out ? 12 : 0)) + 16.0 * B * win_rows * W);
      count_kernel("hz_compose");
      SDM_LAUNCH(hz_compose_kernel, dim3((unsigned)(B * sdm_cdiv(H, SDM_HZ_TH) * sdm_cdiv(W, SDM_HZ_TW))), dim3(256), 0, e->stream,
                 wrap ? (const f32x4*)tplane.p : (const f32x4*)nullptr, d_fg, d_alpha, d_bg, bg_batch, B, H, W, blur, wrap_strength,
                 match ? (const float*)map.p : (const float*)nullptr, match ? (float*)nullptr : d_map_out, d_out, d_fg_out);
      prof_end(e);
    }
    if (wrap) tfree(e, tplane);
    if (match) { tfree(e, map); tfree(e, partials); }
    return 0;
  });
}

// ------------------------------------------------------------------------------------------------
// green-screen shots: screen colour, key, trimap from the key, despill (k_key.h)
// ------------------------------------------------------------------------------------------------
static int key_size_check(sdm_ctx* e, const char* what, int B, int H, int W) {
  if (B <= 0 || H < 1 || W < 1) SDM_FAIL(e, SDM_ERR_INVALID, "%s: bad image size %dx%dx%d", what, B, H, W);
  if (H > SDM_FG_MAX_SIDE || W > SDM_FG_MAX_SIDE || (double)B * H * W > (double)SDM_FG_MAX_PIXELS)
    SDM_FAIL(e, SDM_ERR_INVALID, "%s: %dx%dx%d is too large (sides up to %d, %d pixels in all)", what, B, H, W, SDM_FG_MAX_SIDE, SDM_FG_MAX_PIXELS);
  return 0;
}

/* The histograms (one per slot), {eligible, mode} per slot and the partial sums (16 bytes per run of 4096 pixels) live in the activation arena.  Five
 * launches, whatever the arguments. */
int sdm_screen_colour(sdm_ctx* e, const float* image, int B, int H, int W, int hint, int share, float* screen, int32_t* info, int ptr_kind,
                      void* stream_arg) {
  if (e) dev_use(e->device);
  if (!e || !image || !screen) return SDM_ERR_INVALID;
  TRY(key_size_check(e, "screen colour", B, H, W));
  if (hint < 0 || hint > 2) SDM_FAIL(e, SDM_ERR_INVALID, "screen colour: hint = %d must be 0 (any), 1 (green) or 2 (blue)", hint);
  if (share != 0 && share != 1) SDM_FAIL(e, SDM_ERR_INVALID, "screen colour: share = %d must be 0 or 1", share);
  // a histogram of 4096 ints per slot, cleared and indexed with ints
  if (!share && B > SDM_KEY_MAX_SLOTS)
    SDM_FAIL(e, SDM_ERR_INVALID, "screen colour: B = %d is too large without share (at most %d images, one histogram each)", B, SDM_KEY_MAX_SLOTS);
  static_assert(SDM_KEY_RUN_PX == SDM_KEY_RUN && SDM_KEY_HIST_PX % SDM_KEY_RUN_PX == 0 && SDM_KEY_NBIN == 4096 && (long long)SDM_KEY_MAX_SLOTS * SDM_KEY_NBIN < 2147483647LL,
                "k_key.h is written for these");
  const int slots = share ? 1 : B, per = share ? B : 1, P = per * H * W;             // P <= SDM_FG_MAX_PIXELS
  const int runs = sdm_cdiv(P, SDM_KEY_RUN_PX), hblocks = sdm_cdiv(P, SDM_KEY_HIST_PX);
  const CkColourParams prm = {SDM_KEY_MIN_SUM, SDM_KEY_MIN_SAT, hint};
  const size_t px = (size_t)B * H * W;
  IoSpan in[] = {{(void*)image, px * 12}};
  IoSpan outs[] = {{screen, (size_t)B * 12}, {info, info ? (size_t)B * 16 : 0}};
  return product_call(e, ptr_kind, stream_arg, in, outs, [&]() -> int {
    const float* d_image = (const float*)in[0].p;
    float* d_screen = (float*)outs[0].p; int* d_info = info ? (int*)outs[1].p : nullptr;
    T hist = talloc(e, slots, 1, SDM_KEY_NBIN, 1, 1), mode = talloc(e, slots, 1, 1, 2, 1), partials = talloc(e, slots, runs, 1, 4, 1);
    if (!e->dry) {
      const int vec = P % 4 == 0 && aligned16(d_image) ? 1 : 0;
      const int nh = slots * SDM_KEY_NBIN;
      prof_begin(e, "ck_clear", 0, (double)nh * 4);
      count_kernel("ck_clear");
      SDM_LAUNCH(ck_clear_kernel, dim3((unsigned)sdm_cdiv(nh, 256)), dim3(256), 0, e->stream, (int*)hist.p, nh);
      prof_end(e);
      prof_begin(e, "ck_hist", 0, (double)px * 12);
      count_kernel("ck_hist");
      SDM_LAUNCH(ck_hist_kernel, dim3((unsigned)(slots * hblocks)), dim3(256), 0, e->stream, d_image, slots, P, prm, vec, (int*)hist.p);
      prof_end(e);
      prof_begin(e, "ck_mode", 0, (double)nh * 4);
      count_kernel("ck_mode");
      SDM_LAUNCH(ck_mode_kernel, dim3((unsigned)slots), dim3(256), 0, e->stream, (const int*)hist.p, (int*)mode.p);
      prof_end(e);
      prof_begin(e, "ck_mean", 0, (double)px * 12 + (double)slots * runs * 16);
      count_kernel("ck_mean");
      SDM_LAUNCH(ck_mean_kernel, dim3((unsigned)(slots * runs)), dim3(256), 0, e->stream, d_image, slots, P, prm, vec, (const int*)mode.p,
                 (CkPartial*)partials.p);
      prof_end(e);
      prof_begin(e, "ck_finalize", 0, (double)slots * runs * 16);
      count_kernel("ck_finalize");
      SDM_LAUNCH(ck_finalize_kernel, dim3((unsigned)slots), dim3(64), 0, e->stream, (const CkPartial*)partials.p, (const int*)mode.p, runs, per, d_screen,
                 d_info);
      prof_end(e);
    }
    tfree(e, partials); tfree(e, mode); tfree(e, hist);
    return 0;
  });
}

/* With trimap_bhw: the class bytes, the int16 plane of op_trimap and, without key_bhw, the key live in the activation arena (4 launches); 1 launch
 * otherwise. */
int sdm_chroma_key(sdm_ctx* e, const float* image, const float* screen, int screen_is_plane, int B, int H, int W, float clip_fg, float clip_bg,
                   float sure_fg, float sure_bg, int erode_px, int dilate_px, float despill, float* key, float* trimap, float* despilled, int ptr_kind,
                   void* stream_arg) {
  if (e) dev_use(e->device);
  if (!e || !image || !screen) return SDM_ERR_INVALID;
  TRY(key_size_check(e, "chroma key", B, H, W));
  if (!key && !trimap && !despilled) SDM_FAIL(e, SDM_ERR_INVALID, "chroma key: at least one of key_bhw, trimap_bhw, despilled_bhwc must be given");
  if (screen_is_plane != 0 && screen_is_plane != 1) SDM_FAIL(e, SDM_ERR_INVALID, "chroma key: screen_is_plane = %d must be 0 or 1", screen_is_plane);
  if (!std::isfinite(clip_fg) || !(clip_fg >= 0.0f) || !(clip_fg < 1.0f))
    SDM_FAIL(e, SDM_ERR_INVALID, "chroma key: clip_fg = %g must be a finite number in [0, 1)", (double)clip_fg);
  if (!(clip_bg > clip_fg) || !(clip_bg <= 1.0f)) SDM_FAIL(e, SDM_ERR_INVALID, "chroma key: clip_bg = %g must lie in (clip_fg = %g, 1]", (double)clip_bg, (double)clip_fg);
  if (!std::isfinite(sure_fg) || !(sure_fg >= -1.0f) || !(sure_fg <= 1.0f))
    SDM_FAIL(e, SDM_ERR_INVALID, "chroma key: sure_fg = %g must be a finite number in [-1, 1]", (double)sure_fg);
  if (!(sure_bg >= sure_fg) || !(sure_bg <= 2.0f)) SDM_FAIL(e, SDM_ERR_INVALID, "chroma key: sure_bg = %g must lie in [sure_fg = %g, 2]", (double)sure_bg, (double)sure_fg);
  if (!(despill >= 0.0f) || !(despill <= 1.0f)) SDM_FAIL(e, SDM_ERR_INVALID, "chroma key: despill = %g must lie in [0, 1]", (double)despill);
  if (erode_px < 0 || erode_px > SDM_TRIMAP_MAX_RADIUS || dilate_px < 0 || dilate_px > SDM_TRIMAP_MAX_RADIUS)
    SDM_FAIL(e, SDM_ERR_INVALID, "chroma key: erode_px = %d, dilate_px = %d outside 0 .. %d", erode_px, dilate_px, SDM_TRIMAP_MAX_RADIUS);
  if (trimap) TRY(trimap_check(e, B, H, W, erode_px, dilate_px));      // (the row kernel's grid; cannot fail within SDM_FG_MAX_PIXELS)
  const CkKeyParams prm = {clip_fg, clip_bg, sure_fg, sure_bg, despill, SDM_KEY_MIN_SEP};
  const size_t px = (size_t)B * H * W;
  IoSpan in[] = {{(void*)image, px * 12}, {(void*)screen, screen_is_plane ? px * 12 : (size_t)B * 12}};
  IoSpan outs[] = {{key, key ? px * 4 : 0}, {trimap, trimap ? px * 4 : 0}, {despilled, despilled ? px * 12 : 0}};
  return product_call(e, ptr_kind, stream_arg, in, outs, [&]() -> int {
    const float* d_image = (const float*)in[0].p; const float* d_screen = (const float*)in[1].p;
    float* d_key = key ? (float*)outs[0].p : nullptr; float* d_trimap = trimap ? (float*)outs[1].p : nullptr;
    float* d_desp = despilled ? (float*)outs[2].p : nullptr;
    T cls, dist, keyplane;
    if (trimap) {
      cls = talloc(e, 1, 1, (int)((px + 1) / 2), 1, 0);                 // one byte per pixel
      dist = talloc(e, B, H, W, 1, 0);
      if (!key) keyplane = talloc(e, B, H, W, 1, 1);
    }
    if (!e->dry) {
      float* k_out = d_key ? d_key : (trimap ? (float*)keyplane.p : nullptr);
      const int vec = aligned16(d_image) && (!screen_is_plane || aligned16(d_screen)) && (!k_out || aligned16(k_out)) && (!d_desp || aligned16(d_desp)) ? 1 : 0;
      prof_begin(e, "ck_key", 0, (double)px * ((screen_is_plane ? 24 : 12) + (k_out ? 4 : 0) + (trimap ? 1 : 0) + (d_desp ? 12 : 0)));
      count_kernel("ck_key");
      SDM_LAUNCH(ck_key_kernel, dim3((unsigned)sdm_cdiv(sdm_cdiv((int)px, 4), 256)), dim3(256), 0, e->stream, d_image, d_screen,
                 screen_is_plane, B, H * W, prm, vec, k_out, trimap ? (unsigned char*)cls.p : (unsigned char*)nullptr, d_desp);
      prof_end(e);
      if (trimap) {
        op_trimap(e, k_out, B, H, W, 0.5f, erode_px, dilate_px, (short*)dist.p, d_trimap);
        prof_begin(e, "ck_veto", 0, (double)px * 9);
        count_kernel("ck_veto");
        SDM_LAUNCH(ck_veto_kernel, dim3((unsigned)sdm_cdiv((int)px, 256)), dim3(256), 0, e->stream, d_trimap, (const unsigned char*)cls.p, (long long)px);
        prof_end(e);
      }
    }
    if (trimap) {
      if (!key) tfree(e, keyplane);
      tfree(e, dist); tfree(e, cls);
    }
    return 0;
  });
}

// ------------------------------------------------------------------------------------------------
// mask clean-up: islands, holes, largest component (k_cclabel.h)
// ------------------------------------------------------------------------------------------------
static int clean_check(sdm_ctx* e, int B, int H, int W, float threshold, int min_area, int keep_largest, int max_hole_area, int binarize) {
  if (B <= 0 || H < 1 || W < 1) SDM_FAIL(e, SDM_ERR_INVALID, "clean mask: bad mask size %dx%dx%d", B, H, W);
  // the labels are global pixel indices in an int
  if (H > SDM_FG_MAX_SIDE || W > SDM_FG_MAX_SIDE || (double)B * H * W > (double)SDM_FG_MAX_PIXELS)
    SDM_FAIL(e, SDM_ERR_INVALID, "clean mask: %dx%dx%d is too large (sides up to %d, %d pixels in all)", B, H, W, SDM_FG_MAX_SIDE, SDM_FG_MAX_PIXELS);
  // below 1, so that the 0.0 and 1.0 the call writes lie on the right side of it
  if (!std::isfinite(threshold) || !(threshold >= 0.0f) || !(threshold < 1.0f))
    SDM_FAIL(e, SDM_ERR_INVALID, "clean mask: threshold = %g must be a finite number in [0, 1)", (double)threshold);
  if (min_area < 0 || min_area > SDM_FG_MAX_PIXELS || max_hole_area < 0 || max_hole_area > SDM_FG_MAX_PIXELS)
    SDM_FAIL(e, SDM_ERR_INVALID, "clean mask: min_area = %d, max_hole_area = %d outside 0 .. %d", min_area, max_hole_area, SDM_FG_MAX_PIXELS);
  if ((keep_largest != 0 && keep_largest != 1) || (binarize != 0 && binarize != 1))
    SDM_FAIL(e, SDM_ERR_INVALID, "clean mask: keep_largest = %d, binarize = %d must be 0 or 1", keep_largest, binarize);
  return 0;
}

// one labelling: tile, seam, flatten (3 launches).  Afterwards root[p] is the smallest pixel index of p's component (-1 outside the class) and
// area[root] its pixel count, or >= SDM_CC_BORDER for a stage B component on the image border.
static void op_cc_label(sdm_ctx* e, const float* src, int B, int H, int W, float threshold, bool stage_b, int* label, int* root, int* area, int* sel,
                        int* stats) {
  const double px = (double)B * H * W;
  const int tiles = B * sdm_cdiv(H, SDM_CC_T) * sdm_cdiv(W, SDM_CC_T);
  const int vec = (H * W) % 4 == 0 ? 1 : 0;      // (the planes start on arena boundaries of 256 bytes)
  prof_begin(e, "cc_tile", 0, px * 12);
  count_kernel("cc_tile");
  SDM_LAUNCH(cc_tile_kernel, dim3((unsigned)tiles), dim3(256), 0, e->stream, src, label, area, B, H, W, threshold, stage_b ? 1 : 0, stage_b ? 0 : 1, sel, stats);
  prof_end(e);
  prof_begin(e, "cc_seam", 0, px * 4 * 3 / SDM_CC_T);
  count_kernel("cc_seam");
  SDM_LAUNCH(cc_seam_kernel, dim3((unsigned)tiles), dim3(256), 0, e->stream, label, B, H, W, stage_b ? 0 : 1);
  prof_end(e);
  prof_begin(e, "cc_flatten", 0, px * 8);
  count_kernel("cc_flatten");
  SDM_LAUNCH(cc_flatten_kernel, dim3((unsigned)(B * sdm_cdiv(H * W, SDM_CC_FLAT_PX))), dim3(256), 0, e->stream, (const int*)label, root, area, B, H, W, stage_b ? 1 : 0, vec, stats);
  prof_end(e);
}

/* The label, root and area planes (4 bytes per pixel each) and the selection words live in the activation arena.  Launches: stage A 6 (tile, seam, flatten,
 * select x 2, apply), stage B 4 (tile, seam, flatten, fill); with stage A off the apply launch is the threshold / copy, preceded by one labelling
 * (3 launches) if statistics are asked for. */
int sdm_clean_mask(sdm_ctx* e, const float* mask, int B, int H, int W, float threshold, int min_area, int keep_largest, int max_hole_area, int binarize,
                   float* out, int32_t* stats, int ptr_kind, void* stream_arg) {
  if (e) dev_use(e->device);
  if (!e || !mask || !out) return SDM_ERR_INVALID;
  TRY(clean_check(e, B, H, W, threshold, min_area, keep_largest, max_hole_area, binarize));
  const size_t px = (size_t)B * H * W;
  IoSpan in[] = {{(void*)mask, px * 4}}, outs[] = {{out, px * 4}, {stats, stats ? (size_t)B * SDM_CLEAN_STATS * 4 : 0}};
  const bool stage_a = min_area > 1 || keep_largest, stage_b = max_hole_area > 0;
  const bool label_a = stage_a || stats != nullptr;      // the first statistic is the component count of the input
  return product_call(e, ptr_kind, stream_arg, in, outs, [&]() -> int {
    const float* d_mask = (const float*)in[0].p; float* d_out = (float*)outs[0].p; int* d_stats = (int*)outs[1].p;
    T label, root, area, sel;
    if (label_a || stage_b) { label = talloc(e, B, H, W, 1, 1); root = talloc(e, B, H, W, 1, 1); area = talloc(e, B, H, W, 1, 1); sel = talloc(e, B, 1, 1, 2, 1); }
    if (!e->dry) {
      const int chunks = B * sdm_cdiv(H * W, SDM_CC_PX);
      const int vec = (H * W) % 4 == 0 ? 1 : 0;
      if (label_a) op_cc_label(e, d_mask, B, H, W, threshold, false, (int*)label.p, (int*)root.p, (int*)area.p, (int*)sel.p, d_stats);
      if (stage_a)
        for (int phase = 0; phase < 2; ++phase) {
          prof_begin(e, "cc_select", 0, (double)px * 4);
          count_kernel("cc_select");
          SDM_LAUNCH(cc_select_kernel, dim3((unsigned)chunks), dim3(256), 0, e->stream, (const int*)root.p, (const int*)area.p, B, H, W, phase, vec, (int*)sel.p);
          prof_end(e);
        }
      prof_begin(e, "cc_apply", 0, (double)px * (stage_a ? 12 : 8));
      count_kernel("cc_apply");
      SDM_LAUNCH(cc_apply_kernel, dim3((unsigned)chunks), dim3(256), 0, e->stream, d_mask, (const int*)root.p, (const int*)area.p, (const int*)sel.p, d_out, B, H, W,
                 threshold, stage_a ? 1 : 0, min_area, keep_largest, binarize, (vec && aligned16(d_mask) && aligned16(d_out)) ? 1 : 0, d_stats);
      prof_end(e);
      if (stage_b) {
        op_cc_label(e, d_out, B, H, W, threshold, true, (int*)label.p, (int*)root.p, (int*)area.p, nullptr, nullptr);
        prof_begin(e, "cc_fill", 0, (double)px * 4);
        count_kernel("cc_fill");
        SDM_LAUNCH(cc_fill_kernel, dim3((unsigned)chunks), dim3(256), 0, e->stream, (const int*)root.p, (const int*)area.p, d_out, B, H, W, max_hole_area, vec, d_stats);
        prof_end(e);
      }
    }
    if (label_a || stage_b) { tfree(e, sel); tfree(e, area); tfree(e, root); tfree(e, label); }
    return 0;
  });
}

// ------------------------------------------------------------------------------------------------
// SAD, MSE, Grad and Conn of a matte over the trimap band (k_metrics.h)
// ------------------------------------------------------------------------------------------------
extern "C++" {
template <int R>
static void mm_launch_pixel(sdm_ctx* e, dim3 grid, const float* pred, const float* gt, const float* trimap, int B, int H, int W, const MmWeights& w, float* rec,
                            float* q) {
  auto k = mm_pixel_kernel<R>;
  SDM_SET_SMEM(k, mm_pixel_smem(R));
  SDM_LAUNCH(k, grid, dim3(256), mm_pixel_smem(R), e->stream, pred, gt, trimap, B, H, W, w, rec, q);
}
}

/* The tile records (32 bytes per tile of 64 x 32 pixels) and, with Conn, the plane Q, the label, root and area planes, the level plane (4 bytes per pixel
 * each: 20 in all), the selection words and the run partials live in the activation arena.  2 launches without Conn; with it 63: mm_pixel, ten times
 * (cc_tile, cc_seam, cc_flatten, cc_select x 2, mm_level), mm_conn, mm_finalize - the levels are labelled one after the other on the same three planes. */
int sdm_matte_metrics(sdm_ctx* e, const float* pred, const float* gt, const float* trimap, int B, int H, int W, float grad_sigma, int with_conn,
                      double* stats, int32_t* level, int ptr_kind, void* stream_arg) {
  if (e) dev_use(e->device);
  if (!e || !pred || !gt || !stats) return SDM_ERR_INVALID;
  if (B <= 0 || H < 1 || W < 1) SDM_FAIL(e, SDM_ERR_INVALID, "matte metrics: bad image size %dx%dx%d", B, H, W);
  // (with Conn the labels are global pixel indices in an int; the levels are labelled one at a time, so B H W is the labelled pixel count)
  if (H > SDM_FG_MAX_SIDE || W > SDM_FG_MAX_SIDE || (double)B * H * W > (double)SDM_FG_MAX_PIXELS)
    SDM_FAIL(e, SDM_ERR_INVALID, "matte metrics: %dx%dx%d is too large (sides up to %d, %d pixels in all)", B, H, W, SDM_FG_MAX_SIDE, SDM_FG_MAX_PIXELS);
  if (!std::isfinite(grad_sigma) || !(grad_sigma >= 0.25f) || !(grad_sigma <= 4.0f))
    SDM_FAIL(e, SDM_ERR_INVALID, "matte metrics: grad_sigma = %g must be a finite number in [0.25, 4]", (double)grad_sigma);
  if (with_conn != 0 && with_conn != 1) SDM_FAIL(e, SDM_ERR_INVALID, "matte metrics: with_conn = %d must be 0 or 1", with_conn);
  if (!with_conn && level) SDM_FAIL(e, SDM_ERR_INVALID, "matte metrics: level_bhw needs with_conn = 1");
  static_assert(SDM_MM_R == SDM_MM_MAX_GRAD_RADIUS && SDM_MM_LEVELS == SDM_MM_CONN_LEVELS && SDM_MM_NSTAT == SDM_MM_STATS && SDM_MM_REC >= 8, "k_metrics.h is sized for these");
  // the Gaussian and its derivative, in double from the fp32 sigma, G (x) D scaled to unit L2 norm, rounded to fp32
  MmWeights wts;
  memset(&wts, 0, sizeof(wts));
  {
    const double s = (double)grad_sigma, kPi = 3.14159265358979323846;
    const int r = (int)std::ceil(s * std::sqrt(-2.0 * std::log(std::sqrt(2.0 * kPi) * s * 0.01)));
    wts.r = std::min(SDM_MM_R, std::max(1, r));
    double g[2 * SDM_MM_R + 1], d[2 * SDM_MM_R + 1], ng = 0.0, nd = 0.0;
    for (int k = 0; k <= 2 * wts.r; ++k) {
      const double i = (double)(k - wts.r);
      g[k] = std::exp(-(i * i) / (2.0 * s * s)) / (s * std::sqrt(2.0 * kPi));
      d[k] = -i * g[k] / (s * s);
      ng += g[k] * g[k]; nd += d[k] * d[k];
    }
    const double norm = std::sqrt(std::sqrt(ng * nd));
    for (int k = 0; k <= 2 * wts.r; ++k) { wts.g[k] = (float)(g[k] / norm); wts.d[k] = (float)(d[k] / norm); }
  }
  const size_t px = (size_t)B * H * W;
  const int tiles = sdm_cdiv(H, SDM_MM_TH) * sdm_cdiv(W, SDM_MM_TW), runs = sdm_cdiv(H * W, SDM_MM_RUN_PX);
  IoSpan in[] = {{(void*)pred, px * 4}, {(void*)gt, px * 4}, {(void*)(trimap ? trimap : pred), trimap ? px * 4 : 0}};      // (an absent plane: no bytes, a valid address)
  IoSpan outs[] = {{stats, (size_t)B * SDM_MM_STATS * 8}, {level, level ? px * 4 : 0}};
  return product_call(e, ptr_kind, stream_arg, in, outs, [&]() -> int {
    const float* d_pred = (const float*)in[0].p; const float* d_gt = (const float*)in[1].p; const float* d_tri = trimap ? (const float*)in[2].p : nullptr;
    double* d_stats = (double*)outs[0].p; int* d_level = level ? (int*)outs[1].p : nullptr;
    T rec = talloc(e, B, tiles, 1, SDM_MM_REC, 1), q, label, root, area, lev, sel, part;
    if (with_conn) {
      q = talloc(e, B, H, W, 1, 1); label = talloc(e, B, H, W, 1, 1); root = talloc(e, B, H, W, 1, 1); area = talloc(e, B, H, W, 1, 1);
      lev = talloc(e, B, H, W, 1, 1); sel = talloc(e, B, 1, 1, 2, 1); part = talloc(e, B, runs, 1, 1, 1);
    }
    if (!e->dry) {
      const dim3 pgrid((unsigned)(B * tiles));
      float* d_rec = (float*)rec.p; float* d_q = with_conn ? (float*)q.p : nullptr;
      prof_begin(e, "mm_pixel", 0, (double)px * (d_tri ? 12 : 8) + (double)B * tiles * 32 + (with_conn ? (double)px * 4 : 0.0));
      count_kernel("mm_pixel");
      switch (wts.r) {
        case 1: mm_launch_pixel<1>(e, pgrid, d_pred, d_gt, d_tri, B, H, W, wts, d_rec, d_q); break;
        case 2: mm_launch_pixel<2>(e, pgrid, d_pred, d_gt, d_tri, B, H, W, wts, d_rec, d_q); break;
        case 3: mm_launch_pixel<3>(e, pgrid, d_pred, d_gt, d_tri, B, H, W, wts, d_rec, d_q); break;
        case 4: mm_launch_pixel<4>(e, pgrid, d_pred, d_gt, d_tri, B, H, W, wts, d_rec, d_q); break;
        case 5: mm_launch_pixel<5>(e, pgrid, d_pred, d_gt, d_tri, B, H, W, wts, d_rec, d_q); break;
        case 6: mm_launch_pixel<6>(e, pgrid, d_pred, d_gt, d_tri, B, H, W, wts, d_rec, d_q); break;
        case 7: mm_launch_pixel<7>(e, pgrid, d_pred, d_gt, d_tri, B, H, W, wts, d_rec, d_q); break;
        case 8: mm_launch_pixel<8>(e, pgrid, d_pred, d_gt, d_tri, B, H, W, wts, d_rec, d_q); break;
        default: mm_launch_pixel<9>(e, pgrid, d_pred, d_gt, d_tri, B, H, W, wts, d_rec, d_q); break;
      }
      prof_end(e);
      if (with_conn) {
        const int cc_tiles = B * sdm_cdiv(H, SDM_CC_T) * sdm_cdiv(W, SDM_CC_T), chunks = B * sdm_cdiv(H * W, SDM_CC_PX);
        const int vec = (H * W) % 4 == 0 ? 1 : 0;      // (the planes start on arena boundaries of 256 bytes)
        int* d_label = (int*)label.p; int* d_root = (int*)root.p; int* d_area = (int*)area.p; int* d_sel = (int*)sel.p; int* d_lev = (int*)lev.p;
        for (int k = 1; k <= SDM_MM_LEVELS; ++k) {
          // S_k = { Q >= k } = { Q > k - 0.5 }, 4-connected; the first tile of every image resets the selection words
          prof_begin(e, "cc_tile", 0, (double)px * 12);
          count_kernel("cc_tile");
          SDM_LAUNCH(cc_tile_kernel, dim3((unsigned)cc_tiles), dim3(256), 0, e->stream, (const float*)d_q, d_label, d_area, B, H, W, (float)k - 0.5f, 0, 0, d_sel,
                     (int*)nullptr);
          prof_end(e);
          prof_begin(e, "cc_seam", 0, (double)px * 4 * 3 / SDM_CC_T);
          count_kernel("cc_seam");
          SDM_LAUNCH(cc_seam_kernel, dim3((unsigned)cc_tiles), dim3(256), 0, e->stream, d_label, B, H, W, 0);
          prof_end(e);
          prof_begin(e, "cc_flatten", 0, (double)px * 8);
          count_kernel("cc_flatten");
          SDM_LAUNCH(cc_flatten_kernel, dim3((unsigned)(B * sdm_cdiv(H * W, SDM_CC_FLAT_PX))), dim3(256), 0, e->stream, (const int*)d_label, d_root, d_area, B, H, W,
                     0, vec, (int*)nullptr);
          prof_end(e);
          for (int phase = 0; phase < 2; ++phase) {
            prof_begin(e, "cc_select", 0, (double)px * 4);
            count_kernel("cc_select");
            SDM_LAUNCH(cc_select_kernel, dim3((unsigned)chunks), dim3(256), 0, e->stream, (const int*)d_root, (const int*)d_area, B, H, W, phase, vec, d_sel);
            prof_end(e);
          }
          prof_begin(e, "mm_level", 0, (double)px * (k > 1 ? 12 : 8));
          count_kernel("mm_level");
          SDM_LAUNCH(mm_level_kernel, dim3((unsigned)chunks), dim3(256), 0, e->stream, (const int*)d_root, (const int*)d_sel, d_lev, B, H, W, k, vec);
          prof_end(e);
        }
        prof_begin(e, "mm_conn", 0, (double)px * ((d_tri ? 16 : 12) + (d_level ? 4 : 0)));
        count_kernel("mm_conn");
        SDM_LAUNCH(mm_conn_kernel, dim3((unsigned)(B * runs)), dim3(256), 0, e->stream, d_pred, d_gt, d_tri, (const int*)d_lev, B, H, W, (float*)part.p, d_level);
        prof_end(e);
      }
      prof_begin(e, "mm_finalize", 0, (double)B * tiles * 32 + (with_conn ? (double)B * runs * 4 : 0.0));
      count_kernel("mm_finalize");
      SDM_LAUNCH(mm_finalize_kernel, dim3((unsigned)B), dim3(256), 0, e->stream, (const float*)d_rec, tiles, with_conn ? (const float*)part.p : (const float*)nullptr,
                 runs, B, d_stats);
      prof_end(e);
    }
    if (with_conn) { tfree(e, part); tfree(e, sel); tfree(e, lev); tfree(e, area); tfree(e, root); tfree(e, label); tfree(e, q); }
    tfree(e, rec);
    return 0;
  });
}

// ------------------------------------------------------------------------------------------------
// a box per subject, and the node call over a list of boxes (k_boxes.h)
// ------------------------------------------------------------------------------------------------
static_assert(SDM_BX_SLOTS == SDM_BOXES_MAX - 1 && SDM_BX_LIST == SDM_BOXES_MAX_TOTAL, "box limits");

/* The label, root and area planes (4 bytes per pixel each) and the state (SDM_BX_STRIDE ints per image) live in the activation arena.
 * 8 + 2 (max_boxes - 1) launches, whatever else the arguments are. */
int sdm_subject_boxes(sdm_ctx* e, const float* plane, int B, int H, int W, float roi_threshold, int min_area, int max_boxes, int margin_px, int margin_pct,
                      int square, int32_t* boxes, int32_t* count, int ptr_kind, void* stream_arg) {
  if (e) dev_use(e->device);
  if (!e || !plane || !boxes) return SDM_ERR_INVALID;
  TRY(roi_check(e, "subject boxes", B, H, W, roi_threshold, margin_px, margin_pct, square));
  if (min_area < 0 || min_area > SDM_FG_MAX_PIXELS) SDM_FAIL(e, SDM_ERR_INVALID, "subject boxes: min_area = %d outside 0 .. %d", min_area, SDM_FG_MAX_PIXELS);
  if (max_boxes < 1 || max_boxes > SDM_BOXES_MAX) SDM_FAIL(e, SDM_ERR_INVALID, "subject boxes: max_boxes = %d outside 1 .. %d", max_boxes, SDM_BOXES_MAX);
  const size_t px = (size_t)B * H * W;
  const int K = max_boxes;
  IoSpan in[] = {{(void*)plane, px * 4}}, outs[] = {{boxes, (size_t)B * K * 20}, {count, count ? (size_t)B * 4 : 0}};
  return product_call(e, ptr_kind, stream_arg, in, outs, [&]() -> int {
    const float* d_plane = (const float*)in[0].p; int* d_boxes = (int*)outs[0].p; int* d_count = (int*)outs[1].p;
    T label = talloc(e, B, H, W, 1, 1), root = talloc(e, B, H, W, 1, 1), area = talloc(e, B, H, W, 1, 1), state = talloc(e, B, 1, 1, SDM_BX_STRIDE, 1);
    if (!e->dry) {
      const int chunks = B * sdm_cdiv(H * W, SDM_CC_PX);
      const int vec = (H * W) % 4 == 0 ? 1 : 0;
      const dim3 rgrid((unsigned)(B * sdm_cdiv(H * W, SDM_ROI_PX))), one((unsigned)sdm_cdiv(B, 64));
      const int* d_root = (const int*)root.p; int* d_state = (int*)state.p;
      op_cc_label(e, d_plane, B, H, W, roi_threshold, false, (int*)label.p, (int*)root.p, (int*)area.p, nullptr, nullptr);
      prof_begin(e, "boxes_init", 0, (double)B * SDM_BX_STRIDE * 4);
      count_kernel("boxes_init");
      SDM_LAUNCH(boxes_init_kernel, dim3((unsigned)sdm_cdiv(B * SDM_BX_STRIDE, 256)), dim3(256), 0, e->stream, d_state, B);
      prof_end(e);
      for (int k = 0; k < K - 1; ++k)
        for (int phase = 0; phase < 2; ++phase) {
          prof_begin(e, "boxes_rank", 0, (double)px * 4);
          count_kernel("boxes_rank");
          SDM_LAUNCH(boxes_rank_kernel, dim3((unsigned)chunks), dim3(256), 0, e->stream, d_root, (const int*)area.p, B, H, W, k, phase, min_area, vec, d_state);
          prof_end(e);
        }
      prof_begin(e, "boxes_reduce", 0, (double)px * 4);
      count_kernel("boxes_reduce");
      if (W % 4 == 0) SDM_LAUNCH((boxes_reduce_kernel<true>), rgrid, dim3(256), 0, e->stream, d_root, d_state, B, H, W);
      else SDM_LAUNCH((boxes_reduce_kernel<false>), rgrid, dim3(256), 0, e->stream, d_root, d_state, B, H, W);
      prof_end(e);
      prof_begin(e, "boxes_own", 0, (double)B * SDM_BX_STRIDE * 4);
      count_kernel("boxes_own");
      SDM_LAUNCH(boxes_own_kernel, one, dim3(64), 0, e->stream, d_state, B, H, W, margin_px, margin_pct, square);
      prof_end(e);
      prof_begin(e, "boxes_rest", 0, (double)px * 4);
      count_kernel("boxes_rest");
      if (W % 4 == 0) SDM_LAUNCH((boxes_rest_kernel<true>), rgrid, dim3(256), 0, e->stream, d_root, d_state, B, H, W);
      else SDM_LAUNCH((boxes_rest_kernel<false>), rgrid, dim3(256), 0, e->stream, d_root, d_state, B, H, W);
      prof_end(e);
      prof_begin(e, "boxes_finalize", 0, (double)B * (SDM_BX_STRIDE * 4 + K * 20 + 4));
      count_kernel("boxes_finalize");
      SDM_LAUNCH(boxes_finalize_kernel, one, dim3(64), 0, e->stream, (const int*)d_state, d_boxes, d_count, B, H, W, K, margin_px, margin_pct, square);
      prof_end(e);
    }
    tfree(e, state); tfree(e, area); tfree(e, root); tfree(e, label);
    return 0;
  });
}

/* sdm_apply_matte_node with a model batch of N boxes instead of B frames: forward_impl's node path with the list (an arena tensor of both passes, sanitised
 * on the device) in the place of the frame.  The host knows N, so the sizing pass never sees a data-dependent size. */
int sdm_apply_matte_boxes(sdm_ctx* e, const float* image, const float* trimap, int B, int H, int W, int S, int is_transparent, const int32_t* boxes, int N,
                          int output_mode, int mask_refine, double trimap_constraint, float* alpha, float* matted, int ptr_kind, void* stream_arg) {
  if (e) dev_use(e->device);
  if (!e || !image || !trimap || !boxes || !alpha || !matted) return SDM_ERR_INVALID;
  if (!e->finalized) SDM_FAIL(e, SDM_ERR_STATE, "weights not finalised: call sdm_load_tensor(...) and sdm_finalize_weights first");
  if (output_mode < 0 || output_mode > 2) SDM_FAIL(e, SDM_ERR_INVALID, "unknown output mode %d", output_mode);
  if (N < 1 || N > SDM_BOXES_MAX_TOTAL) SDM_FAIL(e, SDM_ERR_INVALID, "apply matte boxes: N = %d outside 1 .. %d", N, SDM_BOXES_MAX_TOTAL);
  if (S <= 0 || S % 64) SDM_FAIL(e, SDM_ERR_INVALID, "inference size must be a positive multiple of 64 (got %dx%d)", S, S);
  TRY(roi_check(e, "apply matte boxes", B, H, W, 0.0f, 0, 0, 0));
  std::vector<int32_t> it((size_t)N, is_transparent ? 1 : 0);
  NodeTail tail; tail.output_mode = output_mode; tail.mask_refine = mask_refine ? 1 : 0; tail.c = trimap_constraint;
  const size_t px = (size_t)B * H * W;
  IoSpan in[] = {{(void*)image, px * 12}, {(void*)trimap, px * 4}, {(void*)boxes, (size_t)N * 20}};
  IoSpan outs[] = {{alpha, px * 4}, {matted, px * 4 * tail.channels()}};
  return product_call(e, ptr_kind, stream_arg, in, outs, [&]() -> int {
    const float* d_img = (const float*)in[0].p; const float* d_tri = (const float*)in[1].p; const int* d_boxes = (const int*)in[2].p;
    float* d_out = (float*)outs[0].p; float* d_matted = (float*)outs[1].p;
    if (e->dry) TRY(prepare_variants(e, N, it.data(), nullptr, 4, 0));
    T list = talloc(e, N, 1, 1, 5, 1);
    T x16 = talloc(e, 2 * N, S, S, 16, e->act_f32);
    T plane = talloc(e, N, S, S, 1, 1);
    if (!e->dry) {
      const unsigned nb = (unsigned)(((long)N * S * S + 255) / 256);
      void* img16 = x16.p;
      void* tri16 = (unsigned char*)x16.p + (size_t)N * S * S * 16 * fmt_bytes(x16.f32);
      prof_begin(e, "boxes_sanitize", 0, (double)N * 40);
      count_kernel("boxes_sanitize");
      SDM_LAUNCH(boxes_sanitize_kernel, dim3(1), dim3(64), 0, e->stream, d_boxes, (int*)list.p, N, B, H, W);
      prof_end(e);
      // (an upper bound of the bytes: what is read depends on the boxes)
      prof_begin(e, "boxes_prep_image", 0, (double)N * H * W * 12 + (double)N * S * S * 16 * fmt_bytes(x16.f32));
      count_kernel("boxes_prep_image");
      SDM_LAUNCH(boxes_prep_image_kernel, dim3(nb), dim3(256), 0, e->stream, d_img, (const int*)list.p, img16, x16.f32, N, H, W, S);
      prof_end(e);
      prof_begin(e, "boxes_prep_trimap", 0, (double)N * H * W * 4 + (double)N * S * S * (16 * fmt_bytes(x16.f32) + 4));
      count_kernel("boxes_prep_trimap");
      SDM_LAUNCH(boxes_prep_trimap_kernel, dim3(nb), dim3(256), 0, e->stream, d_tri, (const int*)list.p, tri16, x16.f32, (float*)plane.p, N, H, W, S);
      prof_end(e);
    }
    T a;
    TRY(run_model(e, x16, plane, N, S, S, true, &a));
    if (!e->dry) {
      const dim3 fgrid((unsigned)(((long)B * H * W + 255) / 256));
      prof_begin(e, "boxes_paste", 0, (double)px * 4 + (double)N * S * S * 4);
      count_kernel("boxes_paste");
      SDM_LAUNCH(boxes_paste_kernel, fgrid, dim3(256), 0, e->stream, (const float*)a.p, (const int*)list.p, d_out, N, B, H, W, S);
      prof_end(e);
      SDM_LAUNCH(refine_compose_kernel, fgrid, dim3(256), 0, e->stream, d_img, d_tri, d_out, d_matted, (long)B * H * W, tail.output_mode, tail.mask_refine,
                 (float)tail.c, (float)(1.0 - tail.c));
    }
    tfree(e, a); tfree(e, plane); tfree(e, x16); tfree(e, list);
    return 0;
  });
}

// ------------------------------------------------------------------------------------------------
// tiles along the unknown band, and the node call that blends them into the frame (k_tiles.h)
// ------------------------------------------------------------------------------------------------
static_assert(SDM_TL_LIST == SDM_TILES_MAX && SDM_TILES_MAX == SDM_BOXES_MAX_TOTAL && SDM_TL_WORDS * 32 == SDM_TILES_MAX_GRID && SDM_TL_AXIS >= SDM_TILES_MAX_GRID,
              "tile limits");

/* The flag words (SDM_TL_WORDS per image) live in the activation arena.  Three launches, whatever else the arguments are. */
int sdm_band_tiles(sdm_ctx* e, const float* trimap, int B, int H, int W, float band_lo, float band_hi, int tile, int overlap, int max_tiles, int32_t* tiles,
                   int32_t* count, int ptr_kind, void* stream_arg) {
  if (e) dev_use(e->device);
  if (!e || !trimap || !tiles) return SDM_ERR_INVALID;
  TRY(roi_check(e, "band tiles", B, H, W, 0.0f, 0, 0, 0));
  if (!std::isfinite(band_lo) || !std::isfinite(band_hi) || !(band_lo >= 0.0f) || !(band_lo < band_hi) || !(band_hi <= 1.0f))
    SDM_FAIL(e, SDM_ERR_INVALID, "band tiles: band_lo = %g, band_hi = %g must be finite with 0 <= band_lo < band_hi <= 1", (double)band_lo, (double)band_hi);
  if (tile < 16 || tile > SDM_FG_MAX_SIDE) SDM_FAIL(e, SDM_ERR_INVALID, "band tiles: tile = %d outside 16 .. %d", tile, SDM_FG_MAX_SIDE);
  if (overlap < 0 || overlap > tile / 2) SDM_FAIL(e, SDM_ERR_INVALID, "band tiles: overlap = %d outside 0 .. tile / 2 = %d", overlap, tile / 2);
  if (max_tiles < 1 || max_tiles > SDM_TILES_MAX) SDM_FAIL(e, SDM_ERR_INVALID, "band tiles: max_tiles = %d outside 1 .. %d", max_tiles, SDM_TILES_MAX);
  const TilesAxis ay = tiles_axis(H, tile, overlap), ax = tiles_axis(W, tile, overlap);
  if ((long long)ay.n * ax.n > SDM_TILES_MAX_GRID)
    SDM_FAIL(e, SDM_ERR_INVALID, "band tiles: a grid of %d x %d cells is more than %d (tile = %d is too small for %dx%d)", ay.n, ax.n, SDM_TILES_MAX_GRID, tile, H, W);
  const size_t px = (size_t)B * H * W;
  const int K = max_tiles;
  IoSpan in[] = {{(void*)trimap, px * 4}}, outs[] = {{tiles, (size_t)B * K * 20}, {count, count ? (size_t)B * 4 : 0}};
  return product_call(e, ptr_kind, stream_arg, in, outs, [&]() -> int {
    const float* d_plane = (const float*)in[0].p; int* d_tiles = (int*)outs[0].p; int* d_count = (int*)outs[1].p;
    T flags = talloc(e, B, 1, 1, SDM_TL_WORDS, 1);
    if (!e->dry) {
      unsigned int* d_flags = (unsigned int*)flags.p;
      prof_begin(e, "tiles_init", 0, (double)B * SDM_TL_WORDS * 4);
      count_kernel("tiles_init");
      SDM_LAUNCH(tiles_init_kernel, dim3((unsigned)sdm_cdiv(B * SDM_TL_WORDS, 256)), dim3(256), 0, e->stream, d_flags, B);
      prof_end(e);
      const dim3 grid((unsigned)(B * sdm_cdiv(H * W, SDM_ROI_PX)));
      prof_begin(e, "tiles_mark", 0, (double)px * 4);
      count_kernel("tiles_mark");
      if (W % 4 == 0 && aligned16(d_plane)) SDM_LAUNCH((tiles_mark_kernel<true>), grid, dim3(256), 0, e->stream, d_plane, d_flags, B, H, W, band_lo, band_hi, ay, ax);
      else SDM_LAUNCH((tiles_mark_kernel<false>), grid, dim3(256), 0, e->stream, d_plane, d_flags, B, H, W, band_lo, band_hi, ay, ax);
      prof_end(e);
      prof_begin(e, "tiles_list", 0, (double)B * (SDM_TL_WORDS * 4 + K * 20 + 4));
      count_kernel("tiles_list");
      SDM_LAUNCH(tiles_list_kernel, dim3((unsigned)sdm_cdiv(B, 64)), dim3(64), 0, e->stream, (const unsigned int*)d_flags, d_tiles, d_count, B, K, ay, ax);
      prof_end(e);
    }
    tfree(e, flags);
    return 0;
  });
}

/* sdm_apply_matte_boxes with the weighted blend of k_tiles.h in the place of the maximum, and a base for the pixels outside every tile.  N = 0 runs the blend
 * and the tail only: no list, no model input, no model pass. */
int sdm_apply_matte_tiles(sdm_ctx* e, const float* image, const float* trimap, int B, int H, int W, int S, int is_transparent, const int32_t* tiles, int N,
                          int feather_px, const float* base, int output_mode, int mask_refine, double trimap_constraint, float* alpha, float* matted,
                          int ptr_kind, void* stream_arg) {
  if (e) dev_use(e->device);
  if (!e || !image || !trimap || !alpha || !matted) return SDM_ERR_INVALID;
  if (!e->finalized) SDM_FAIL(e, SDM_ERR_STATE, "weights not finalised: call sdm_load_tensor(...) and sdm_finalize_weights first");
  if (output_mode < 0 || output_mode > 2) SDM_FAIL(e, SDM_ERR_INVALID, "unknown output mode %d", output_mode);
  if (N < 0 || N > SDM_TILES_MAX) SDM_FAIL(e, SDM_ERR_INVALID, "apply matte tiles: N = %d outside 0 .. %d", N, SDM_TILES_MAX);
  if (N > 0 && !tiles) SDM_FAIL(e, SDM_ERR_INVALID, "apply matte tiles: tiles_n5 is NULL with N = %d", N);
  if (feather_px < 0 || feather_px > SDM_TILES_MAX_FEATHER)
    SDM_FAIL(e, SDM_ERR_INVALID, "apply matte tiles: feather_px = %d outside 0 .. %d", feather_px, SDM_TILES_MAX_FEATHER);
  if (S <= 0 || S % 64) SDM_FAIL(e, SDM_ERR_INVALID, "inference size must be a positive multiple of 64 (got %dx%d)", S, S);
  TRY(roi_check(e, "apply matte tiles", B, H, W, 0.0f, 0, 0, 0));
  std::vector<int32_t> it((size_t)std::max(N, 1), is_transparent ? 1 : 0);
  NodeTail tail; tail.output_mode = output_mode; tail.mask_refine = mask_refine ? 1 : 0; tail.c = trimap_constraint;
  const size_t px = (size_t)B * H * W;
  // (an empty list and an absent base: no bytes behind a valid address)
  IoSpan in[] = {{(void*)image, px * 12}, {(void*)trimap, px * 4}, {(void*)(N ? (const void*)tiles : (const void*)image), (size_t)N * 20},
                 {(void*)(base ? base : image), base ? px * 4 : 0}};
  IoSpan outs[] = {{alpha, px * 4}, {matted, px * 4 * tail.channels()}};
  return product_call(e, ptr_kind, stream_arg, in, outs, [&]() -> int {
    const float* d_img = (const float*)in[0].p; const float* d_tri = (const float*)in[1].p; const int* d_tiles = (const int*)in[2].p;
    const float* d_base = base ? (const float*)in[3].p : nullptr;
    float* d_out = (float*)outs[0].p; float* d_matted = (float*)outs[1].p;
    T list, x16, plane, a;
    if (N) {
      if (e->dry) TRY(prepare_variants(e, N, it.data(), nullptr, 4, 0));
      list = talloc(e, N, 1, 1, 5, 1);
      x16 = talloc(e, 2 * N, S, S, 16, e->act_f32);
      plane = talloc(e, N, S, S, 1, 1);
      if (!e->dry) {
        const unsigned nb = (unsigned)(((long)N * S * S + 255) / 256);
        void* img16 = x16.p;
        void* tri16 = (unsigned char*)x16.p + (size_t)N * S * S * 16 * fmt_bytes(x16.f32);
        prof_begin(e, "boxes_sanitize", 0, (double)N * 40);
        count_kernel("boxes_sanitize");
        SDM_LAUNCH(boxes_sanitize_kernel, dim3(1), dim3(64), 0, e->stream, d_tiles, (int*)list.p, N, B, H, W);
        prof_end(e);
        // (an upper bound of the bytes: what is read depends on the tiles)
        prof_begin(e, "boxes_prep_image", 0, (double)N * H * W * 12 + (double)N * S * S * 16 * fmt_bytes(x16.f32));
        count_kernel("boxes_prep_image");
        SDM_LAUNCH(boxes_prep_image_kernel, dim3(nb), dim3(256), 0, e->stream, d_img, (const int*)list.p, img16, x16.f32, N, H, W, S);
        prof_end(e);
        prof_begin(e, "boxes_prep_trimap", 0, (double)N * H * W * 4 + (double)N * S * S * (16 * fmt_bytes(x16.f32) + 4));
        count_kernel("boxes_prep_trimap");
        SDM_LAUNCH(boxes_prep_trimap_kernel, dim3(nb), dim3(256), 0, e->stream, d_tri, (const int*)list.p, tri16, x16.f32, (float*)plane.p, N, H, W, S);
        prof_end(e);
      }
      TRY(run_model(e, x16, plane, N, S, S, true, &a));
    }
    if (!e->dry) {
      const dim3 bgrid((unsigned)(B * sdm_cdiv(H, SDM_TL_BH) * sdm_cdiv(W, SDM_TL_BW))), fgrid((unsigned)(((long)B * H * W + 255) / 256));
      // (an upper bound of the bytes: the write, a base or trimap value per pixel, the slots once)
      prof_begin(e, "tiles_blend", 0, (double)px * 8 + (double)N * S * S * 4);
      count_kernel("tiles_blend");
      SDM_LAUNCH(tiles_blend_kernel, bgrid, dim3(256), 0, e->stream, N ? (const float*)a.p : (const float*)nullptr, N ? (const int*)list.p : (const int*)nullptr,
                 d_tri, d_base, d_out, N, B, H, W, S, feather_px);
      prof_end(e);
      SDM_LAUNCH(refine_compose_kernel, fgrid, dim3(256), 0, e->stream, d_img, d_tri, d_out, d_matted, (long)B * H * W, tail.output_mode, tail.mask_refine,
                 (float)tail.c, (float)(1.0 - tail.c));
    }
    if (N) { tfree(e, a); tfree(e, plane); tfree(e, x16); tfree(e, list); }
    return 0;
  });
}

// ------------------------------------------------------------------------------------------------
// the cut-out on a canvas (k_canvas.h)
// ------------------------------------------------------------------------------------------------
/* The raw extrema, the box and the placements live in the activation arena, and with a shadow the layer (16 bytes per canvas pixel) and one blur plane (4).
 * Five launches without a shadow, seven with one, whatever else the arguments are. */
int sdm_compose_canvas(sdm_ctx* e, const float* fg, const float* alpha, int B, int H, int W, float roi_threshold, int canvas_h, int canvas_w, int fill_pct,
                       int valign, int bg_mode, const float* bg_rgb3, const float* bg_image, int bg_batch, float shadow_opacity, float shadow_sigma,
                       int shadow_dy, int shadow_dx, float* out, int out_channels, int32_t* place_out, int ptr_kind, void* stream_arg) {
  if (e) dev_use(e->device);
  if (!e || !fg || !alpha || !out) return SDM_ERR_INVALID;
  TRY(roi_check(e, "compose canvas", B, H, W, roi_threshold, 0, 0, 0));
  if (canvas_h < 1 || canvas_w < 1 || canvas_h > SDM_FG_MAX_SIDE || canvas_w > SDM_FG_MAX_SIDE || (double)B * canvas_h * canvas_w > (double)SDM_FG_MAX_PIXELS)
    SDM_FAIL(e, SDM_ERR_INVALID, "compose canvas: canvas %dx%dx%d outside sides 1 .. %d, %d pixels in all", B, canvas_h, canvas_w, SDM_FG_MAX_SIDE,
             SDM_FG_MAX_PIXELS);
  if (fill_pct < 1 || fill_pct > 100) SDM_FAIL(e, SDM_ERR_INVALID, "compose canvas: fill_pct = %d outside 1 .. 100", fill_pct);
  if (valign < 0 || valign > 2) SDM_FAIL(e, SDM_ERR_INVALID, "compose canvas: valign = %d outside 0 .. 2", valign);
  if (bg_mode < 0 || bg_mode > 2) SDM_FAIL(e, SDM_ERR_INVALID, "compose canvas: bg_mode = %d outside 0 .. 2", bg_mode);
  if (out_channels != 3 && out_channels != 4) SDM_FAIL(e, SDM_ERR_INVALID, "compose canvas: out_channels = %d, must be 3 or 4", out_channels);
  if (bg_mode == 0 && out_channels != 4) SDM_FAIL(e, SDM_ERR_INVALID, "compose canvas: out_channels = 3 needs a background (bg_mode 1 or 2)");
  if (bg_mode == 1 && !bg_rgb3) SDM_FAIL(e, SDM_ERR_INVALID, "compose canvas: bg_mode 1 needs bg_rgb3");
  if (bg_mode == 2 && (!bg_image || (bg_batch != 1 && bg_batch != B)))
    SDM_FAIL(e, SDM_ERR_INVALID, "compose canvas: bg_mode 2 needs bg_image with bg_batch = 1 or %d (got %d)", B, bg_batch);
  if (!std::isfinite(shadow_opacity) || !(shadow_opacity >= 0.0f) || !(shadow_opacity <= 1.0f))
    SDM_FAIL(e, SDM_ERR_INVALID, "compose canvas: shadow_opacity = %g must be a finite number in [0, 1]", (double)shadow_opacity);
  const bool shadow = shadow_opacity > 0.0f;
  if (shadow && (!std::isfinite(shadow_sigma) || !(shadow_sigma > 0.0f) || !(shadow_sigma <= (float)SDM_CANVAS_MAX_SHADOW_SIGMA)))
    SDM_FAIL(e, SDM_ERR_INVALID, "compose canvas: shadow_sigma = %g must be a finite number in (0, %d]", (double)shadow_sigma, SDM_CANVAS_MAX_SHADOW_SIGMA);
  if (shadow_dy < -SDM_CANVAS_MAX_SHADOW_OFFSET || shadow_dy > SDM_CANVAS_MAX_SHADOW_OFFSET || shadow_dx < -SDM_CANVAS_MAX_SHADOW_OFFSET ||
      shadow_dx > SDM_CANVAS_MAX_SHADOW_OFFSET)
    SDM_FAIL(e, SDM_ERR_INVALID, "compose canvas: shadow offset (%d, %d) outside -%d .. %d", shadow_dy, shadow_dx, SDM_CANVAS_MAX_SHADOW_OFFSET,
             SDM_CANVAS_MAX_SHADOW_OFFSET);
  static_assert(SDM_CANVAS_R == SDM_CANVAS_MAX_SHADOW_RADIUS && 3 * SDM_CANVAS_MAX_SHADOW_SIGMA <= SDM_CANVAS_MAX_SHADOW_RADIUS, "shadow limits");
  CanvasBlur blur;
  memset(&blur, 0, sizeof(blur));
  if (shadow) {      // w_i = exp(-i^2 / (2 sigma^2)) / sum, in double, rounded to fp32
    const double s = (double)shadow_sigma;
    blur.r = std::min(SDM_CANVAS_R, std::max(1, (int)std::ceil(3.0 * s)));
    double g[2 * SDM_CANVAS_R + 1], sum = 0.0;
    for (int k = 0; k <= 2 * blur.r; ++k) { const double i = (double)(k - blur.r); g[k] = std::exp(-(i * i) / (2.0 * s * s)); sum += g[k]; }
    for (int k = 0; k <= 2 * blur.r; ++k) blur.w[k] = (float)(g[k] / sum);
  }
  CanvasBg bg;
  bg.mode = bg_mode; bg.batch = bg_batch; bg.image = nullptr;
  for (int c = 0; c < 3; ++c) bg.rgb[c] = bg_mode == 1 ? bg_rgb3[c] : 0.0f;
  const size_t px = (size_t)B * H * W, cpx = (size_t)B * canvas_h * canvas_w;
  // (an absent background image is an empty span behind a valid pointer: the staging copies 0 bytes of it)
  IoSpan in[] = {{(void*)fg, px * 12}, {(void*)alpha, px * 4}, {(void*)(bg_mode == 2 ? bg_image : fg), bg_mode == 2 ? (size_t)bg_batch * canvas_h * canvas_w * 12 : 0}};
  IoSpan outs[] = {{out, cpx * 4 * out_channels}, {place_out, place_out ? (size_t)B * 32 : 0}};
  return product_call(e, ptr_kind, stream_arg, in, outs, [&]() -> int {
    const float* d_fg = (const float*)in[0].p; const float* d_alpha = (const float*)in[1].p;
    float* d_out = (float*)outs[0].p; int* d_place_out = (int*)outs[1].p;
    CanvasBg dbg = bg;
    if (bg_mode == 2) dbg.image = (const float*)in[2].p;
    T raw = talloc(e, B, 1, 1, 4, 1), box = talloc(e, B, 1, 1, 4, 1), place = talloc(e, B, 1, 1, 8, 1);
    T layer, tplane;
    if (shadow) { layer = talloc(e, B, canvas_h, canvas_w, 4, 1); tplane = talloc(e, B, canvas_h, canvas_w, 1, 1); }
    if (!e->dry) {
      op_roi_box(e, d_alpha, B, H, W, roi_threshold, 0, 0, 0, (int*)raw.p, (int*)box.p);
      prof_begin(e, "canvas_fit", 0, (double)B * 48);
      count_kernel("canvas_fit");
      SDM_LAUNCH(canvas_fit_kernel, dim3((unsigned)sdm_cdiv(B, 64)), dim3(64), 0, e->stream, (const int*)box.p, (int*)place.p, d_place_out, B, canvas_h, canvas_w,
                 fill_pct, valign);
      prof_end(e);
      const dim3 blk(256);
      const double bg_bytes = bg_mode == 2 ? 12.0 : 0.0, out_bytes = 4.0 * out_channels;
      if (!shadow) {
        // per canvas pixel: the store and the background; the box (at most 16 bytes per source pixel) comes through L1 / L2
        prof_begin(e, "canvas_compose", 0, (double)cpx * (out_bytes + bg_bytes) + (double)px * 16);
        count_kernel("canvas_compose");
        const int vec = aligned16(d_out) ? 1 : 0;
        if (out_channels == 4)
          SDM_LAUNCH((canvas_compose_kernel<4>), dim3((unsigned)sdm_cdiv((int)cpx, 256)), blk, 0, e->stream, d_fg, d_alpha, (const int*)place.p, B, H, W, canvas_h,
                     canvas_w, dbg, vec, d_out);
        else
          SDM_LAUNCH((canvas_compose_kernel<3>), dim3((unsigned)sdm_cdiv((int)((cpx + 3) / 4), 256)), blk, 0, e->stream, d_fg, d_alpha, (const int*)place.p, B, H, W,
                     canvas_h, canvas_w, dbg, vec, d_out);
        prof_end(e);
      } else {
        prof_begin(e, "canvas_place", 0, (double)cpx * 16 + (double)px * 16);
        count_kernel("canvas_place");
        SDM_LAUNCH(canvas_place_kernel, dim3((unsigned)sdm_cdiv((int)cpx, 256)), blk, 0, e->stream, d_fg, d_alpha, (const int*)place.p, B, H, W, canvas_h, canvas_w,
                   (float*)layer.p);
        prof_end(e);
        prof_begin(e, "canvas_blur_rows", 0, (double)cpx * 20);      // A_s arrives in 16-byte pixels
        count_kernel("canvas_blur_rows");
        SDM_LAUNCH(canvas_blur_rows_kernel, dim3((unsigned)(B * canvas_h * sdm_cdiv(canvas_w, SDM_CANVAS_ROW_W))), blk, 0, e->stream, (const float*)layer.p, B,
                   canvas_h, canvas_w, shadow_dx, blur, (float*)tplane.p);
        prof_end(e);
        const int th = canvas_tile_h(blur.r);
        const dim3 grid((unsigned)(B * sdm_cdiv(canvas_h, th) * sdm_cdiv(canvas_w, SDM_CANVAS_TW)));
        prof_begin(e, "canvas_blur_compose", 0, (double)cpx * (16 + 4.0 * (th + 2 * blur.r) / th + out_bytes + bg_bytes));
        count_kernel("canvas_blur_compose");
        const int vec = (aligned16(d_out) && (out_channels == 4 || canvas_w % 4 == 0)) ? 1 : 0;
        if (out_channels == 4)
          SDM_LAUNCH((canvas_blur_compose_kernel<4>), grid, blk, canvas_blur_smem(blur.r), e->stream, (const float*)layer.p, (const float*)tplane.p, B, canvas_h,
                     canvas_w, shadow_dy, shadow_opacity, blur, dbg, vec, d_out);
        else
          SDM_LAUNCH((canvas_blur_compose_kernel<3>), grid, blk, canvas_blur_smem(blur.r), e->stream, (const float*)layer.p, (const float*)tplane.p, B, canvas_h,
                     canvas_w, shadow_dy, shadow_opacity, blur, dbg, vec, d_out);
        prof_end(e);
      }
    }
    if (shadow) { tfree(e, tplane); tfree(e, layer); }
    tfree(e, place); tfree(e, box); tfree(e, raw);
    return 0;
  });
}

/* The distance field on its own (k_distance.h).  The class words, the carries and the column distances live in the activation arena.  Four launches,
 * whatever the arguments. */
int sdm_distance_field(sdm_ctx* e, const float* plane, int B, int H, int W, float threshold, int32_t* field, int ptr_kind, void* stream_arg) {
  if (e) dev_use(e->device);
  if (!e || !plane || !field) return SDM_ERR_INVALID;
  TRY(df_check(e, "distance field", B, H, W, threshold));
  const size_t bytes = (size_t)B * H * W * 4;
  IoSpan in[] = {{(void*)plane, bytes}}, out[] = {{field, bytes}};
  return product_call(e, ptr_kind, stream_arg, in, out, [&]() -> int {
    DfScratch s = df_talloc(e, B, H, W);
    if (!e->dry) {
      DfEmit emit;
      memset(&emit, 0, sizeof(emit));
      emit.field = (int32_t*)out[0].p;
      op_distance(e, (const float*)in[0].p, B, H, W, threshold, s, 0, emit);
    }
    df_tfree(e, s);
    return 0;
  });
}

/* Grow, shrink and feather a mask: the row pass of the distance field applies the ramp, the field itself is never stored.  Four launches. */
int sdm_offset_mask(sdm_ctx* e, const float* mask, int B, int H, int W, float threshold, float offset_px, float feather_px, float* out_mask, int ptr_kind,
                    void* stream_arg) {
  if (e) dev_use(e->device);
  if (!e || !mask || !out_mask) return SDM_ERR_INVALID;
  TRY(df_check(e, "offset mask", B, H, W, threshold));
  if (!std::isfinite(offset_px) || !(offset_px >= -(float)SDM_DF_MAX_OFFSET) || !(offset_px <= (float)SDM_DF_MAX_OFFSET))
    SDM_FAIL(e, SDM_ERR_INVALID, "offset mask: offset_px = %g must be a finite number within +-%d", (double)offset_px, SDM_DF_MAX_OFFSET);
  if (!std::isfinite(feather_px) || !(feather_px >= 1.0f) || !(feather_px <= (float)SDM_DF_MAX_FEATHER))
    SDM_FAIL(e, SDM_ERR_INVALID, "offset mask: feather_px = %g must be a finite number in [1, %d]", (double)feather_px, SDM_DF_MAX_FEATHER);
  const size_t bytes = (size_t)B * H * W * 4;
  IoSpan in[] = {{(void*)mask, bytes}}, out[] = {{out_mask, bytes}};
  return product_call(e, ptr_kind, stream_arg, in, out, [&]() -> int {
    DfScratch s = df_talloc(e, B, H, W);
    if (!e->dry) {
      DfEmit emit;
      memset(&emit, 0, sizeof(emit));
      emit.out = (float*)out[0].p; emit.offset = offset_px; emit.feather = feather_px;
      op_distance(e, (const float*)in[0].p, B, H, W, threshold, s, 1, emit);
    }
    df_tfree(e, s);
    return 0;
  });
}

/* A stroke along the silhouette of a straight-alpha cut-out, composed with it in the row pass of the distance field of the alpha.  Four launches. */
int sdm_outline(sdm_ctx* e, const float* fg, const float* alpha, int B, int H, int W, float edge_threshold, int position, float width_px, float softness_px,
                const float* rgb3, float opacity, float* out_rgb, float* out_alpha, int ptr_kind, void* stream_arg) {
  if (e) dev_use(e->device);
  if (!e || !fg || !alpha || !rgb3 || !out_rgb || !out_alpha) return SDM_ERR_INVALID;
  TRY(df_check(e, "outline", B, H, W, edge_threshold));
  if (position < 0 || position > 2) SDM_FAIL(e, SDM_ERR_INVALID, "outline: position = %d outside 0 .. 2", position);
  if (!std::isfinite(width_px) || !(width_px > 0.0f) || !(width_px <= (float)SDM_OUTLINE_MAX_WIDTH))
    SDM_FAIL(e, SDM_ERR_INVALID, "outline: width_px = %g must be a finite number in (0, %d]", (double)width_px, SDM_OUTLINE_MAX_WIDTH);
  if (!std::isfinite(softness_px) || !(softness_px >= 1.0f) || !(softness_px <= (float)SDM_DF_MAX_FEATHER))
    SDM_FAIL(e, SDM_ERR_INVALID, "outline: softness_px = %g must be a finite number in [1, %d]", (double)softness_px, SDM_DF_MAX_FEATHER);
  if (!std::isfinite(opacity) || !(opacity >= 0.0f) || !(opacity <= 1.0f))
    SDM_FAIL(e, SDM_ERR_INVALID, "outline: opacity = %g must be a finite number in [0, 1]", (double)opacity);
  for (int c = 0; c < 3; ++c)
    if (!std::isfinite(rgb3[c])) SDM_FAIL(e, SDM_ERR_INVALID, "outline: rgb3[%d] = %g must be finite", c, (double)rgb3[c]);
  const size_t px = (size_t)B * H * W;
  IoSpan in[] = {{(void*)fg, px * 12}, {(void*)alpha, px * 4}}, out[] = {{out_rgb, px * 12}, {out_alpha, px * 4}};
  return product_call(e, ptr_kind, stream_arg, in, out, [&]() -> int {
    DfScratch s = df_talloc(e, B, H, W);
    if (!e->dry) {
      DfEmit emit;
      memset(&emit, 0, sizeof(emit));
      emit.fg = (const float*)in[0].p; emit.alpha = (const float*)in[1].p; emit.out_rgb = (float*)out[0].p; emit.out_alpha = (float*)out[1].p;
      emit.position = position; emit.softness = softness_px; emit.opacity = opacity;
      emit.hi = position == 0 ? width_px : (position == 1 ? width_px * 0.5f : 0.0f);
      emit.lo = position == 1 ? -width_px * 0.5f : -width_px;      // (not read for position 0: no lower edge)
      for (int c = 0; c < 3; ++c) emit.rgb[c] = rgb3[c];
      op_distance(e, emit.alpha, B, H, W, edge_threshold, s, 2, emit);
    }
    df_tfree(e, s);
    return 0;
  });
}

int sdm_synchronize(sdm_ctx* e) {
  if (e) dev_use(e->device);
  if (!e) return SDM_ERR_INVALID;
  SDM_CHECK_DEV(e, dev_sync(e->stream));
#ifndef SDM_EMU
  float ms = 0.f;
  if (hipEventElapsedTime(&ms, e->ev0, e->ev1) == hipSuccess) e->last_ms = ms;
  if (!e->prof.empty()) {
    std::map<std::string, sdm_ctx::ProfAgg> agg;
    e->prof_dump = "kernel,ms,gflop,mbytes,desc\n";
    for (auto& r : e->prof) {
      float t = 0.f;
      (void)hipEventElapsedTime(&t, r.e0, r.e1);
      char line[512];
      snprintf(line, sizeof(line), "%s,%.4f,%.3f,%.3f,%s\n", r.name.c_str(), t, r.flops * 1e-9, r.bytes * 1e-6, r.desc.c_str());
      e->prof_dump += line;
      auto& a = agg[r.name];
      a.name = r.name; a.ms += t; a.n += 1; a.flops += r.flops; a.bytes += r.bytes;
      (void)hipEventDestroy(r.e0); (void)hipEventDestroy(r.e1);
    }
    e->prof.clear();
    e->prof_agg.clear();
    for (auto& kv : agg) e->prof_agg.push_back(kv.second);
  }
#endif
  return SDM_OK;
}

float sdm_last_forward_ms(sdm_ctx* e) { return e ? e->last_ms : 0.f; }

int sdm_profile_enable(sdm_ctx* e, int on) { if (!e) return SDM_ERR_INVALID; e->prof_on = on != 0; return SDM_OK; }
int sdm_profile_count(sdm_ctx* e) { return e ? (int)e->prof_agg.size() : 0; }
const char* sdm_profile_dump(sdm_ctx* e) { return e ? e->prof_dump.c_str() : ""; }
int sdm_profile_get(sdm_ctx* e, int i, const char** name, float* ms, int64_t* launches, double* flops, double* bytes) {
  if (!e || i < 0 || i >= (int)e->prof_agg.size()) return SDM_ERR_INVALID;
  auto& a = e->prof_agg[(size_t)i];
  if (name) *name = a.name.c_str();
  if (ms) *ms = a.ms;
  if (launches) *launches = a.n;
  if (flops) *flops = a.flops;
  if (bytes) *bytes = a.bytes;
  return SDM_OK;
}

}  // extern "C"

// the single-operator test hooks and the lab / bench helpers of the C ABI: no product path calls them (same translation unit, as the k_*.h kernels)
#include "sdm_hooks.h"
