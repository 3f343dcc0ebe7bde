// k_metrics.h - the matting literature's four numbers over the trimap band: SAD, MSE, Grad, Conn (sdm_matte_metrics in include/sdmatte.h, which is the
// normative text; DESIGN.md 4, "matte metrics").
//
//   p, g = clamp01(pred, gt; NaN -> 0);  R = { |trimap - 0.5| < 0.25 } (the whole frame without a trimap);  e = p - g
// Launches, whatever B, H, W and the content:
//   mm_pixel_kernel<R>  (always) a block of 256 threads owns 64 x 32 pixels of one image: lane = column, a wave owns 8 rows.  p and g of the tile plus a halo
//                       of r (replicate padding resolved while loading: the index is clamped, the filter loops know no border) go into LDS once.  Pass 1, the
//                       inner sums over the rows i = -r .. r: a thread owns one column of 8 output rows, reads its 8 + 2 r inputs once and keeps both sums
//                       (weights G and D) of both planes in registers - p and g travel as a pair, so every multiply and add is a packed one; the 2 r halo
//                       columns are spread over the block's first threads.  The four planes of inner sums go to LDS (as two planes of pairs); pass 2, the
//                       outer sums over the columns j = -r .. r, reads them back with lane = column (consecutive 8-byte pairs:
//                       conflict-free for every row stride).  r is a template parameter (1 .. 9), so both passes are unrolled and the weights sit in
//                       scalar registers.  Then the magnitudes, the six terms, and the tile's record: per thread its 8 pixels top to bottom, over the wave
//                       a butterfly of shuffles, over the four waves in wave order - a fixed tree, no atomics.  With Conn the plane Q (the number of
//                       thresholds t_1 .. t_10 that min(p, g) reaches, as a float: the source plane of cc_tile_kernel) is written as well.  No product is
//                       fused into an addition anywhere: m(p) - m(g) is a difference of nearly equal numbers, and on regular images the rounding of a
//                       fused filter is systematic enough to move the Grad sum by several 1e-6 relative against the unfused fp32 order of the header.
//   cc_tile / cc_seam / cc_flatten / cc_select x 2 (k_cclabel.h, unchanged) and mm_level_kernel, once per level k = 1 .. 10 (Conn only): S_k = { Q > k - 0.5 }
//                       is labelled 4-connected, its largest component (smallest root on a tie) selected, and a pixel whose level is k - 1 and whose root is
//                       the selected one moves to level k.  An empty S_k selects no root.
//   mm_conn_kernel      (Conn only) a block owns a run of SDM_MM_RUN_PX = 4096 consecutive pixels of one image: one read of pred, gt, trimap and the level;
//                       the Conn terms of a thread's 16 pixels in index order, then the same tree; level_bhw is written when asked for.
//   mm_finalize_kernel  (always) a block per image: the records pass through LDS, thread s sums statistic s over the image's tiles (runs for Conn) in fp64
//                       in ascending order.
// No load leaves the tensors: halo indices are clamped into the frame, pixels of a tile beyond the frame are computed from clamped values and take no part
// in any sum or store, runs are cut at H W.
#pragma once
#include "sdm_common.h"
#include "k_guided.h"      // gf_alpha
#include "k_cclabel.h"     // cc_load4, SDM_CC_PX

#define SDM_MM_TW 64                                   // tile columns: a wave's lanes
#define SDM_MM_TH 32                                   // tile rows: 4 waves x 8
#define SDM_MM_ROWS 8                                  // output rows of a wave
#define SDM_MM_R 9                                     // the largest radius (SDM_MM_MAX_GRAD_RADIUS)
#define SDM_MM_REC 8                                   // words of a tile's record: n (a float: at most 2048, exact), sad, sse, grad, max|e|, frame sad, frame sse, unused
#define SDM_MM_NSTAT 8                                 // statistics per image (SDM_MM_STATS); mm_finalize_kernel needs SDM_MM_REC >= 8: column 7 carries the Conn runs
#define SDM_MM_RUN_PX 4096                             // pixels of a run of mm_conn_kernel: 256 threads x 16
#define SDM_MM_LEVELS 10                               // SDM_MM_CONN_LEVELS
#define SDM_MM_THETA 0.15f                             // SDM_MM_CONN_THETA

struct MmWeights { int r; float g[2 * SDM_MM_R + 1]; float d[2 * SDM_MM_R + 1]; };      // g[k], d[k] = weight of offset k - r (double on the host, rounded to fp32)

// dynamic LDS of mm_pixel_kernel<R>: p and g with their halo, then the four planes of inner sums
SDM_HD_INLINE size_t mm_pixel_smem(int r) {
  const size_t sw = SDM_MM_TW + 2 * r;
  return (2 * (size_t)(SDM_MM_TH + 2 * r) * sw + 4 * (size_t)SDM_MM_TH * sw) * sizeof(float);
}

SDM_DEV_INLINE bool mm_in_region(float t) { return fabsf(t - 0.5f) < 0.25f; }      // (NaN compares false: outside)

// the sum of v over the block in a fixed order: the wave by a butterfly, the four waves in wave order; returned in thread 0 (red: 4 floats of LDS)
SDM_DEV_INLINE float mm_block_sum(float v, float* red) {
#pragma clang fp contract(off)
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
  __syncthreads();                                     // the last use of red is behind every thread
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

// pass 1 for one column `c` of the strip and the 8 output rows from `row0`: the inner sums with G into vg2, with D into vd2.  A value is the pair (p, g): the
// two planes go through every instruction together (packed fp32 arithmetic, 8-byte LDS accesses); rows of sw pairs.
template <int R>
SDM_DEV_INLINE void mm_inner_sums(const f32x2* __restrict__ s2, int sw, int row0, int c, const MmWeights& w, f32x2* __restrict__ vg2, f32x2* __restrict__ vd2) {
#pragma clang fp contract(off)
  f32x2 in[SDM_MM_ROWS + 2 * R];
#pragma unroll
  for (int s = 0; s < SDM_MM_ROWS + 2 * R; ++s) in[s] = s2[(row0 + s) * sw + c];      // input row row0 + s = output row row0 + s - R
#pragma unroll
  for (int o = 0; o < SDM_MM_ROWS; ++o) {
    f32x2 a = {0.0f, 0.0f}, b = {0.0f, 0.0f};
#pragma unroll
    for (int k = 0; k <= 2 * R; ++k) {                 // ascending i = k - R
      a += w.g[k] * in[o + k];
      b += w.d[k] * in[o + k];
    }
    vg2[(row0 + o) * sw + c] = a;
    vd2[(row0 + o) * sw + c] = b;
  }
}

// grid: B * ceil(H / 32) * ceil(W / 64) blocks of 256 threads, mm_pixel_smem(R) bytes of dynamic LDS.  trimap: null = the whole frame.  rec: [B][tiles][8].
// q_out: null without Conn, else [B][H][W].
template <int R>
__global__ __launch_bounds__(256) void mm_pixel_kernel(const float* __restrict__ pred, const float* __restrict__ gt, const float* __restrict__ trimap, int B, int H,
                                                       int W, MmWeights w, float* __restrict__ rec, float* __restrict__ q_out) {
  SDM_DYN_SMEM(smem);
  SDM_SHARED float red[4][6];
  SDM_SHARED int redn[4];
  constexpr int SW = SDM_MM_TW + 2 * R, SH = SDM_MM_TH + 2 * R;
  f32x2* s2 = (f32x2*)smem;                            // [SH][SW] pairs (p, g)
  f32x2* vg2 = s2 + SH * SW;                           // [32][SW] pairs each: the inner sums with G, with D
  f32x2* vd2 = vg2 + SDM_MM_TH * SW;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int nbx = (W + SDM_MM_TW - 1) / SDM_MM_TW, nby = (H + SDM_MM_TH - 1) / SDM_MM_TH;
  const int blk = blockIdx.x;
  const int b = blk / (nbx * nby), tile = blk - b * (nbx * nby);
  const int y0 = (tile / nbx) * SDM_MM_TH, x0 = (tile % nbx) * SDM_MM_TW;
  const size_t base = (size_t)b * H * W;

  // the tile and its halo; a pixel beyond the frame takes the nearest pixel of the frame.  Every load of the thread is issued before the first one is used
  // (one latency per block, not one per row), the trimap values of its 8 pixels among them.
  constexpr int NEL = SH * SW, NIT = (NEL + 255) / 256;
  float lp[NIT], lg[NIT], tv[SDM_MM_ROWS];
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int idx = it * 256 + tid, row = idx / SW, c = idx - row * SW;
    lp[it] = lg[it] = 0.0f;
    if (idx < NEL) {
      const size_t at = base + (size_t)min(max(y0 - R + row, 0), H - 1) * W + min(max(x0 - R + c, 0), W - 1);
      lp[it] = pred[at];
      lg[it] = gt[at];
    }
  }
#pragma unroll
  for (int o = 0; o < SDM_MM_ROWS; ++o) {
    const int y = y0 + wv * SDM_MM_ROWS + o;
    tv[o] = (trimap && y < H && x0 + lane < W) ? trimap[base + (size_t)y * W + x0 + lane] : 0.5f;      // (no trimap: a plane of 0.5)
  }
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int idx = it * 256 + tid;
    if (idx < NEL) s2[idx] = f32x2{gf_alpha(lp[it]), gf_alpha(lg[it])};
  }
  __syncthreads();
  mm_inner_sums<R>(s2, SW, wv * SDM_MM_ROWS, lane, w, vg2, vd2);
  if (tid < 2 * R * 4) mm_inner_sums<R>(s2, SW, (tid / (2 * R)) * SDM_MM_ROWS, SDM_MM_TW + tid % (2 * R), w, vg2, vd2);
  __syncthreads();

  const int x = x0 + lane;
  int n = 0;
  float sad = 0.0f, sse = 0.0f, grad = 0.0f, mx = 0.0f, fsad = 0.0f, fsse = 0.0f;
#pragma unroll
  for (int o = 0; o < SDM_MM_ROWS; ++o) {
    const int ly = wv * SDM_MM_ROWS + o, y = y0 + ly;
    f32x2 ax = {0.0f, 0.0f}, ay = {0.0f, 0.0f};       // (a_x, a_y) of (p, g)
#pragma unroll
    for (int k = 0; k <= 2 * R; ++k) {                 // ascending j = k - R; column lane + k of the strip is column x + j
#pragma clang fp contract(off)
      const int at = ly * SW + lane + k;
      ax += w.d[k] * vg2[at];
      ay += w.g[k] * vd2[at];
    }
    if (y < H && x < W) {                              // (y: the same for the whole wave)
#pragma clang fp contract(off)
      const f32x2 pg = s2[(ly + R) * SW + lane + R];
      const float p = pg[0], g = pg[1];
      const float px = ax[0], py = ay[0], gx = ax[1], gy = ay[1];
      const float e = p - g, ae = fabsf(e), ee = e * e;
      const float mp = sqrtf(px * px + py * py), mg = sqrtf(gx * gx + gy * gy), dm = mp - mg;
      const size_t at = base + (size_t)y * W + x;
      fsad += ae; fsse += ee;
      if (mm_in_region(tv[o])) { ++n; sad += ae; sse += ee; grad += dm * dm; mx = fmaxf(mx, ae); }
      if (q_out) {
        const float c = fminf(p, g);
        int q = 0;
#pragma unroll
        for (int k = 1; k <= SDM_MM_LEVELS; ++k) q += (c >= (float)k / 10.0f) ? 1 : 0;
        q_out[at] = (float)q;
      }
    }
  }
  // the tile's record: the wave by a butterfly, the four waves in wave order
  float v[6] = {sad, sse, grad, fsad, fsse, mx};
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
#pragma clang fp contract(off)
    n += __shfl_xor(n, d);
#pragma unroll
    for (int k = 0; k < 5; ++k) v[k] += __shfl_xor(v[k], d);
    v[5] = fmaxf(v[5], __shfl_xor(v[5], d));
  }
  if (lane == 0) {
    redn[wv] = n;
#pragma unroll
    for (int k = 0; k < 6; ++k) red[wv][k] = v[k];
  }
  __syncthreads();
  if (tid < SDM_MM_REC) {
    float* out = rec + ((size_t)b * nbx * nby + tile) * SDM_MM_REC;
    if (tid == 0) out[0] = (float)(((redn[0] + redn[1]) + redn[2]) + redn[3]);     // (at most 2048: exact)
    else if (tid == 4) out[4] = fmaxf(fmaxf(red[0][5], red[1][5]), fmaxf(red[2][5], red[3][5]));
    else if (tid == 7) out[7] = 0.0f;
    else {
      const int k = tid <= 3 ? tid - 1 : tid - 2;      // words 1, 2, 3 = sad, sse, grad; 5, 6 = the frame's sad, sse
      out[tid] = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
    }
  }
}

// grid: B * ceil(H W / 1024) blocks of 256 threads (no block spans two images).  After level k: L = k where L was k - 1 and the pixel's root is the root
// selected for S_k (sel[2 b + 1]; 0x7FFFFFFF when S_k is empty, which no root equals).  k == 1 also initialises the plane: L is not read.
__global__ __launch_bounds__(256) void mm_level_kernel(const int* __restrict__ root, const int* __restrict__ sel, int* __restrict__ level, int B, int H, int W,
                                                       int k, int vec) {
  const int HW = H * W, nchunk = (HW + SDM_CC_PX - 1) / SDM_CC_PX;
  const int b = blockIdx.x / nchunk, chunk = blockIdx.x % nchunk;
  if (b >= B) return;
  const int base = b * HW, pl0 = chunk * SDM_CC_PX + threadIdx.x * 4;
  if (pl0 >= HW) return;
  const int keep = sel[2 * b + 1];
  int r[4], l[4] = {0, 0, 0, 0};
  cc_load4(root, base, pl0, HW, vec, r);
  if (k > 1) cc_load4(level, base, pl0, HW, vec, l);
#pragma unroll
  for (int j = 0; j < 4; ++j) if (l[j] == k - 1 && r[j] >= 0 && r[j] == keep) l[j] = k;
  if (vec && pl0 + 3 < HW) {
    i32x4 q; q[0] = l[0]; q[1] = l[1]; q[2] = l[2]; q[3] = l[3];
    *(i32x4*)(level + base + pl0) = q;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) if (pl0 + j < HW) level[base + pl0 + j] = l[j];
  }
}

// phi(a) = 1 - d [d >= theta], d = a - l
SDM_DEV_INLINE float mm_phi(float a, float l) {
#pragma clang fp contract(off)
  const float d = a - l;
  return 1.0f - (d >= SDM_MM_THETA ? d : 0.0f);
}

// grid: B * ceil(H W / 4096) blocks of 256 threads.  partials: [B][runs].  level_out: null or [B][H][W].
__global__ __launch_bounds__(256) void mm_conn_kernel(const float* __restrict__ pred, const float* __restrict__ gt, const float* __restrict__ trimap,
                                                      const int* __restrict__ level, int B, int H, int W, float* __restrict__ partials,
                                                      int* __restrict__ level_out) {
#pragma clang fp contract(off)
  SDM_SHARED float red[4];
  const int HW = H * W, runs = (HW + SDM_MM_RUN_PX - 1) / SDM_MM_RUN_PX;
  const int b = blockIdx.x / runs, run = blockIdx.x - b * runs;
  const size_t base = (size_t)b * HW;
  float s = 0.0f;
#pragma unroll 4
  for (int j = 0; j < SDM_MM_RUN_PX / 256; ++j) {
    const int i = run * SDM_MM_RUN_PX + j * 256 + (int)threadIdx.x;
    if (i < HW) {
      const int L = level[base + i];
      if (level_out) level_out[base + i] = L;
      if (!trimap || mm_in_region(trimap[base + i])) {
        const float l = (float)L / 10.0f;
        s += fabsf(mm_phi(gf_alpha(pred[base + i]), l) - mm_phi(gf_alpha(gt[base + i]), l));
      }
    }
  }
  s = mm_block_sum(s, red);
  if (threadIdx.x == 0) partials[(size_t)b * runs + run] = s;
}

// grid: B blocks of 256 threads.  stats[b][s] = the sum of statistic s over the image's units in ascending order in fp64 (the counts are floats, so n is
// such a sum too, and exact; max|e|: the maximum).
// The records pass through LDS SDM_MM_FIN_CHUNK units at a time, loaded by the whole block; thread s < 8 then adds its statistic's column one unit after the
// other, so the chain of fp64 additions waits for LDS reads that do not depend on it, never for global memory.  conn: null without Conn (stats[b][4] = 0);
// its runs take the same way through column 7 (the records' unused word).
#define SDM_MM_FIN_CHUNK 1024
#define SDM_MM_FIN_LD (SDM_MM_FIN_CHUNK + 8)           // column stride: the 8 words of a record land on 8 different banks
__global__ __launch_bounds__(256) void mm_finalize_kernel(const float* __restrict__ rec, int tiles, const float* __restrict__ conn, int runs, int B,
                                                         double* __restrict__ stats) {
  SDM_SHARED float buf[SDM_MM_REC * SDM_MM_FIN_LD];
  const int b = blockIdx.x, tid = threadIdx.x;
  if (b >= B) return;                                  // (the whole block)
  const float* r = rec + (size_t)b * tiles * SDM_MM_REC;
  double v = 0.0;
  float m = 0.0f;
  const int word = tid == 0 ? 0 : (tid <= 3 ? tid : (tid == 4 ? 7 : (tid == 5 ? 4 : tid - 1)));      // statistic -> record word (4: Conn, column 7)
  const int units = max(tiles, conn ? runs : 0);
  for (int u0 = 0; u0 < units; u0 += SDM_MM_FIN_CHUNK) {
    const int nt = min(SDM_MM_FIN_CHUNK, tiles - u0), nr = conn ? min(SDM_MM_FIN_CHUNK, runs - u0) : 0;      // (may be <= 0)
    __syncthreads();                                   // the last chunk has been read
    float ld[SDM_MM_FIN_CHUNK * SDM_MM_REC / 256];     // every load of the chunk is issued before the first one is used
#pragma unroll
    for (int j = 0; j < SDM_MM_FIN_CHUNK * SDM_MM_REC / 256; ++j) {
      const int i = j * 256 + tid;
      ld[j] = i < nt * SDM_MM_REC ? r[(size_t)u0 * SDM_MM_REC + i] : 0.0f;
    }
#pragma unroll
    for (int j = 0; j < SDM_MM_FIN_CHUNK * SDM_MM_REC / 256; ++j) {
      const int i = j * 256 + tid;
      if (i < nt * SDM_MM_REC && (i & (SDM_MM_REC - 1)) != 7) buf[(i & (SDM_MM_REC - 1)) * SDM_MM_FIN_LD + (i >> 3)] = ld[j];
    }
    for (int i = tid; i < nr; i += 256) buf[7 * SDM_MM_FIN_LD + i] = conn[(size_t)b * runs + u0 + i];
    __syncthreads();
    if (tid < SDM_MM_NSTAT) {
      const float* col = buf + word * SDM_MM_FIN_LD;
      const int cnt = tid == 4 ? nr : nt;
      // one loop for all eight threads, sum and maximum side by side (two loops behind a branch would run one after the other); thread 5 keeps the
      // maximum, the others the sum
#pragma unroll 8
      for (int t = 0; t < cnt; ++t) {
        const float x = col[t];
        v += (double)x;
        m = fmaxf(m, x);
      }
    }
  }
  if (tid < SDM_MM_NSTAT) stats[(size_t)b * SDM_MM_NSTAT + tid] = tid == 5 ? (double)m : v;
}
