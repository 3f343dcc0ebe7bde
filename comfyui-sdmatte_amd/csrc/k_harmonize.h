// k_harmonize.h - the cut-out in its new scene: colour match and light wrap (sdm_harmonize in include/sdmatte.h, which is the normative text; DESIGN.md 4,
// "harmonize").
//
//   a = clamp01(alpha, NaN -> 0);  Bg = image b of the background, or image 0 when bg_batch == 1;  opponent coordinates o = (l, p, q) of a colour:
//   l = ((r + g) + b) / 3, p = r - g, q = (r + g) / 2 - b
// Up to FOUR launches; which of them run depends on the strengths alone:
//   hz_stats_kernel     (match on) a block owns one run of SDM_HZ_RUN = 4096 consecutive pixels of one image, a thread 4 groups of 4 pixels, two in
//                       flight at a time (ts_load: 16-byte loads when H W % 4 == 0 and the tensors are aligned, scalar loads otherwise, one arithmetic path).  The 14 fp32 sums of the run
//                       (sum a, a o_c(F), (a o_c(F)) o_c(F), o_c(Bg), o_c(Bg)^2, the pixel count) are formed in the thread (its 16 pixels in index order),
//                       over the wave by a butterfly of shuffles, over the four waves in LDS in wave order: a fixed tree, no atomics.  One row of 14
//                       floats per run goes into the arena.
//   hz_finalize_kernel  (match on) one wave per image: lane i sums the partials of runs i, i + 64, ... in fp64, thread k < 14 sums the 64 lane sums of
//                       sum k in lane order, thread 0 forms the moments and the map (fp64, rounded to fp32 at the end) and writes its 12 floats.
//   hz_rows_kernel      (wrap on) T(y, x) = sum over i = -r .. r (ascending) of w_i X(y, x + i), X = ((1 - a) Bg.r, (1 - a) Bg.g, (1 - a) Bg.b, 1 - a),
//                       0 beyond the frame.  A wave owns 256 columns of one row: its 256 + 2 r4 pixels of X (r4 = r rounded up to 4, so that every load is
//                       an aligned run of 4 pixels) go through a wave-private LDS strip once, a lane sums the taps of columns lane, lane + 64, lane + 128,
//                       lane + 192 (every 16-byte LDS read and every global store is 64 consecutive pixels).  No block barrier.
//   hz_compose_kernel   (always) a block of 256 threads owns 64 x 64 output pixels: lane = column, a wave owns 16 rows and keeps their column sums
//                       (Wr, Wg, Wb, m) in registers.  The rows y0 - r .. y0 + 63 + r of T that exist go through LDS 8 at a time; a source row at
//                       distance j = sr - y from output row y adds wz[j] T(sr, x), where wz is the weight table in LDS padded with zeros on both sides
//                       (a wave runs its 16 rows without a branch; a term with weight 0 adds 0 and changes no bit).  Source rows arrive in ascending
//                       order, so the terms of a pixel are summed in ascending j.  The epilogue applies the map, the wrap and the composition; colours and
//                       results cross wave-private LDS strips as in dof_gather_kernel, so global memory sees consecutive dwords and there is one path for
//                       every alignment.  With the match off the map is the identity, formed in the kernel (and written to map_out by the first block of
//                       an image); with the wrap off the kernel gets no plane and skips the window loop.
// The exact shortcut for tiles whose window holds no subject or no visible background is NOT built.
// No load leaves the tensors: runs are fetched only where they lie in the image (a run of the vector path is whole by construction), every LDS index lies in
// its strip (see the kernels), the window rows are clipped to the frame, and the epilogue touches only pixels of the tile that exist.
#pragma once
#include "sdm_common.h"
#include "k_guided.h"      // gf_alpha
#include "k_temporal.h"    // ts_load

#define SDM_HZ_RUN_PX 4096                                              // SDM_HZ_RUN: pixels of a run = 256 threads x 4 groups x 4 pixels
#define SDM_HZ_NSUM 14                                                  // sums per run
#define SDM_HZ_R 48                                                     // the largest wrap radius: ceil(3 SDM_HZ_MAX_WRAP_SIGMA)
#define SDM_HZ_SEG 256                                                  // columns of a wave of hz_rows_kernel
#define SDM_HZ_STRIP (SDM_HZ_SEG + 2 * SDM_HZ_R)                        // ... and the pixels of its LDS strip at the largest radius (48 % 4 == 0)
#define SDM_HZ_TW 64                                                    // tile columns of hz_compose_kernel: a wave's lanes
#define SDM_HZ_TH 64                                                    // tile rows: 4 waves x 16
#define SDM_HZ_ROWS 16                                                  // output rows of a wave
#define SDM_HZ_CH 8                                                     // rows of T in LDS at a time
#define SDM_HZ_WZ (2 * SDM_HZ_R + 2 * (SDM_HZ_ROWS - 1) + 1)            // entries of the zero-padded weight table

struct HzBlur { int r; float w[2 * SDM_HZ_R + 1]; };                    // w[k] = weight of offset k - r, k = 0 .. 2r (computed in double on the host)
struct HzParams { float luma, chroma, contrast, wrap; };                // the four strengths as they crossed the C ABI

SDM_DEV_INLINE void hz_opponent(float r, float g, float b, float (&o)[3]) {
#pragma clang fp contract(off)
  o[0] = ((r + g) + b) / 3.0f;
  o[1] = r - g;
  o[2] = (r + g) / 2.0f - b;
}

// grid: B * ceil(H W / 4096) blocks of 256 threads.  vec: H W % 4 == 0 and fg, alpha, bg 16-byte aligned.  partials: [B][runs][14].
__global__ __launch_bounds__(256) void hz_stats_kernel(const float* __restrict__ fg, const float* __restrict__ alpha, const float* __restrict__ bg,
                                                       int bg_batch, int B, int H, int W, int vec, float* __restrict__ partials) {
#pragma clang fp contract(off)
  SDM_SHARED float red[4][SDM_HZ_NSUM];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int HW = H * W, runs = (HW + SDM_HZ_RUN_PX - 1) / SDM_HZ_RUN_PX;
  const int b = blockIdx.x / runs, run = blockIdx.x - b * runs;
  const size_t fbase = (size_t)b * HW, bbase = (size_t)(bg_batch == 1 ? 0 : b) * HW;
  float s[SDM_HZ_NSUM];
#pragma unroll
  for (int k = 0; k < SDM_HZ_NSUM; ++k) s[k] = 0.0f;
  for (int half = 0; half < 2; ++half) {                                // two groups' loads are in flight together
    float cf[2][12], cb[2][12], al[2][4];
    int npx[2];
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const int i = run * SDM_HZ_RUN_PX + ((2 * half + it) * 256 + tid) * 4;      // pixel index in the image: a multiple of 4
      npx[it] = max(0, min(4, HW - i));
#pragma unroll
      for (int k = 0; k < 12; ++k) cf[it][k] = cb[it][k] = 0.0f;
#pragma unroll
      for (int k = 0; k < 4; ++k) al[it][k] = 0.0f;
      if (npx[it] > 0) {
        float dummy[4];
        ts_load(fg, alpha, fbase + i, npx[it], vec != 0, true, cf[it], al[it]);
        ts_load(bg, alpha, bbase + i, npx[it], vec != 0, false, cb[it], dummy);
      }
    }
#pragma unroll
    for (int it = 0; it < 2; ++it) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (k < npx[it]) {
          const float a = gf_alpha(al[it][k]);
          float of[3], ob[3];
          hz_opponent(cf[it][3 * k], cf[it][3 * k + 1], cf[it][3 * k + 2], of);
          hz_opponent(cb[it][3 * k], cb[it][3 * k + 1], cb[it][3 * k + 2], ob);
          s[0] += a;
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const float ao = a * of[c];
            s[1 + c] += ao;
            s[4 + c] += ao * of[c];
            s[7 + c] += ob[c];
            s[10 + c] += ob[c] * ob[c];
          }
          s[13] += 1.0f;
        }
      }
    }
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
#pragma unroll
    for (int k = 0; k < SDM_HZ_NSUM; ++k) s[k] += __shfl_xor(s[k], d);
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < SDM_HZ_NSUM; ++k) red[wv][k] = s[k];
  }
  __syncthreads();
  if (tid < SDM_HZ_NSUM) partials[((size_t)b * runs + run) * SDM_HZ_NSUM + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

// M = I + sum over c of (g_c - 1) P_c and t = sum over c of h_c k_c, in fp64: the projectors of the opponent coordinates (include/sdmatte.h)
SDM_DEV_INLINE void hz_map_from_moments(const double (&S)[SDM_HZ_NSUM], HzParams prm, double var_floor, double max_gain, double min_weight, float (&map)[12]) {
  double M[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}, t[3] = {0.0, 0.0, 0.0};
  if (S[0] >= min_weight) {
    const double Pm[3][9] = {{1.0 / 3, 1.0 / 3, 1.0 / 3, 1.0 / 3, 1.0 / 3, 1.0 / 3, 1.0 / 3, 1.0 / 3, 1.0 / 3},
                             {0.5, -0.5, 0.0, -0.5, 0.5, 0.0, 0.0, 0.0, 0.0},
                             {1.0 / 6, 1.0 / 6, -1.0 / 3, 1.0 / 6, 1.0 / 6, -1.0 / 3, -1.0 / 3, -1.0 / 3, 2.0 / 3}};
    const double kv[3][3] = {{1.0, 1.0, 1.0}, {0.5, -0.5, 0.0}, {1.0 / 3, 1.0 / 3, -2.0 / 3}};
    const double sc[3] = {(double)prm.luma, (double)prm.chroma, (double)prm.chroma};
    for (int c = 0; c < 3; ++c) {
      const double mf = S[1 + c] / S[0], vf = S[4 + c] / S[0] - mf * mf;
      const double mb = S[7 + c] / S[13], vb = S[10 + c] / S[13] - mb * mb;
      // (a variance from raw moments may come out a rounding error below 0: clamped first, as the header says)
      double rho = sqrt(((vb > 0.0 ? vb : 0.0) + var_floor) / ((vf > 0.0 ? vf : 0.0) + var_floor));
      rho = rho < 1.0 / max_gain ? 1.0 / max_gain : (rho > max_gain ? max_gain : rho);
      const double g = 1.0 + (double)prm.contrast * sc[c] * (rho - 1.0);
      const double h = mf * (1.0 - g) + sc[c] * (mb - mf);
      for (int k = 0; k < 9; ++k) M[k] += (g - 1.0) * Pm[c][k];
      for (int k = 0; k < 3; ++k) t[k] += h * kv[c][k];
    }
  }
  for (int k = 0; k < 9; ++k) map[k] = (float)M[k];
  for (int k = 0; k < 3; ++k) map[9 + k] = (float)t[k];
}

// grid: B blocks of 64 threads.  map: [B][12] in the arena; map_out: the caller's copy, or null.
__global__ __launch_bounds__(64) void hz_finalize_kernel(const float* __restrict__ partials, int B, int runs, HzParams prm, double var_floor, double max_gain,
                                                         double min_weight, float* __restrict__ map, float* __restrict__ map_out) {
  SDM_SHARED double lanes[SDM_HZ_NSUM][64];
  SDM_SHARED double tot[SDM_HZ_NSUM];
  const int lane = threadIdx.x, b = blockIdx.x;
  double acc[SDM_HZ_NSUM];
  for (int k = 0; k < SDM_HZ_NSUM; ++k) acc[k] = 0.0;
  for (int j = lane; j < runs; j += 64) {
    const float* p = partials + ((size_t)b * runs + j) * SDM_HZ_NSUM;
    for (int k = 0; k < SDM_HZ_NSUM; ++k) acc[k] += (double)p[k];
  }
  for (int k = 0; k < SDM_HZ_NSUM; ++k) lanes[k][lane] = acc[k];
  __syncthreads();
  if (lane < SDM_HZ_NSUM) {
    double s = 0.0;
    for (int i = 0; i < 64; ++i) s += lanes[lane][i];
    tot[lane] = s;
  }
  __syncthreads();
  if (lane == 0) {
    double S[SDM_HZ_NSUM];
    for (int k = 0; k < SDM_HZ_NSUM; ++k) S[k] = tot[k];
    float m[12];
    hz_map_from_moments(S, prm, var_floor, max_gain, min_weight, m);
    for (int k = 0; k < 12; ++k) {
      map[b * 12 + k] = m[k];
      if (map_out) map_out[b * 12 + k] = m[k];
    }
  }
}

// acc += w v (contraction allowed: the blur sums are not part of the bit-level contract beyond "a sum of zeros is zero")
SDM_DEV_INLINE void hz_axpy(f32x4& acc, float w, const f32x4& v) { acc += w * v; }

// grid: ceil(B * H * ceil(W / 256) / 4) blocks of 256 threads.  vec: W % 4 == 0 and bg, alpha 16-byte aligned.  tplane: [B][H][W][4].
__global__ __launch_bounds__(256) void hz_rows_kernel(const float* __restrict__ alpha, const float* __restrict__ bg, int bg_batch, int B, int H, int W,
                                                      HzBlur blur, int vec, f32x4* __restrict__ tplane) {
  SDM_SHARED f32x4 strip[4][SDM_HZ_STRIP];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int r = blur.r, r4 = (r + 3) & ~3;                              // r4 <= SDM_HZ_R
  const int nseg = (W + SDM_HZ_SEG - 1) / SDM_HZ_SEG;
  const long long units = (long long)B * H * nseg, u = (long long)blockIdx.x * 4 + wv;
  if (u >= units) return;                                               // (the whole wave; nothing below crosses waves)
  const long long row = u / nseg;                                       // b * H + y
  const int b = (int)(row / H), y = (int)(row - (long long)b * H);
  const int x0 = (int)(u - row * nseg) * SDM_HZ_SEG;
  const size_t arow = (size_t)row * W, brow = ((size_t)(bg_batch == 1 ? 0 : b) * H + y) * W;
  const int xw = x0 - r4, nrun = (SDM_HZ_SEG + 2 * r4) / 4;             // the strip's first column (a multiple of 4, may be negative) and its runs (<= 88)
  f32x4* st = strip[wv];
  for (int t = lane; t < nrun; t += 64) {                               // at most two runs per lane
    const int xs = xw + 4 * t;
    const int npx = xs >= 0 ? max(0, min(4, W - xs)) : 0;               // xs < 0: the whole run lies left of the frame
    float c[12], a[4] = {1.0f, 1.0f, 1.0f, 1.0f}, dummy[4];
#pragma unroll
    for (int k = 0; k < 12; ++k) c[k] = 0.0f;
    if (npx > 0) {
      ts_load(bg, alpha, brow + xs, npx, vec != 0, false, c, dummy);
      if (vec) { const f32x4 av = *(const f32x4*)(alpha + arow + xs); a[0] = av[0]; a[1] = av[1]; a[2] = av[2]; a[3] = av[3]; }
      else {
#pragma unroll
        for (int k = 0; k < 4; ++k) if (k < npx) a[k] = alpha[arow + xs + k];
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
#pragma clang fp contract(off)
      const float v = 1.0f - gf_alpha(a[k]);
      f32x4 X = {v * c[3 * k], v * c[3 * k + 1], v * c[3 * k + 2], v};
      if (k >= npx) X = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
      st[4 * t + k] = X;                                                // 4 t + k < 4 nrun <= SDM_HZ_STRIP
    }
  }
  SDM_WAVE_SYNC();
  f32x4 acc[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) acc[k] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  const int o = r4 - r + lane;                                          // strip index of column x0 + lane at tap -r; o + 192 + 2 r <= 255 + r4 + r < 4 nrun
#pragma unroll 2
  for (int i = 0; i <= 2 * r; ++i) {
    const float w = blur.w[i];
#pragma unroll
    for (int k = 0; k < 4; ++k) hz_axpy(acc[k], w, st[o + 64 * k + i]);
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int x = x0 + lane + 64 * k;
    if (x < W) tplane[arow + x] = acc[k];
  }
}

// grid: B * ceil(H / 64) * ceil(W / 64) blocks of 256 threads.  tplane: null without the wrap.  map: [B][12], null = the identity (then map_id_out, unless
// null, gets the identity's 12 floats per image from the image's first block).  fg_out: null or [B][H][W][3].
__global__ __launch_bounds__(256) void hz_compose_kernel(const f32x4* __restrict__ tplane, const float* __restrict__ fg, const float* __restrict__ alpha,
                                                         const float* __restrict__ bg, int bg_batch, int B, int H, int W, HzBlur blur, float wrap,
                                                         const float* __restrict__ map, float* __restrict__ map_id_out, float* __restrict__ out,
                                                         float* __restrict__ fg_out) {
#pragma clang fp contract(off)
  SDM_SHARED f32x4 win[SDM_HZ_CH * SDM_HZ_TW];
  SDM_SHARED float wz[SDM_HZ_WZ + 3];
  SDM_SHARED float strips[4][4][3 * SDM_HZ_TW];                         // per wave: F, Bg, out, fg_out
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int nbx = (W + SDM_HZ_TW - 1) / SDM_HZ_TW, nby = (H + SDM_HZ_TH - 1) / SDM_HZ_TH;
  const int blk = blockIdx.x;
  const int b = blk / (nbx * nby), y0 = ((blk / nbx) % nby) * SDM_HZ_TH, x0 = (blk % nbx) * SDM_HZ_TW;
  const int x = x0 + lane;                                              // lanes right of the image sum zeros and store nothing
  const int yw = y0 + SDM_HZ_ROWS * wv;                                 // this wave's first output row
  const int r = blur.r;
  f32x4 acc[SDM_HZ_ROWS];
#pragma unroll
  for (int i = 0; i < SDM_HZ_ROWS; ++i) acc[i] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

  if (tplane) {
    // wz[j + r + 15] = w_j for |j| <= r, 0 for the 15 entries on either side: 2 r + 31 <= SDM_HZ_WZ entries
    for (int k = tid; k < 2 * r + 2 * (SDM_HZ_ROWS - 1) + 1; k += 256) {
      const int j = k - (SDM_HZ_ROWS - 1);
      wz[k] = (j >= 0 && j <= 2 * r) ? blur.w[j] : 0.0f;
    }
    const int r_lo = max(0, y0 - r), r_hi = min(H - 1, y0 + SDM_HZ_TH - 1 + r);
    for (int c0 = r_lo; c0 <= r_hi; c0 += SDM_HZ_CH) {
      const int nrows = min(SDM_HZ_CH, r_hi - c0 + 1);
      __syncthreads();                                                  // every read of the window's last content is behind us (and wz is written)
      for (int idx = tid; idx < nrows * SDM_HZ_TW; idx += 256) {
        const int row = idx >> 6, gx = x0 + (idx & 63);
        f32x4 v = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        if (gx < W) v = tplane[((size_t)b * H + c0 + row) * W + gx];    // (c0 + row lies in [0, H))
        win[idx] = v;
      }
      __syncthreads();
      for (int rr = 0; rr < nrows; ++rr) {
        const int d0 = c0 + rr - yw;                                    // j of the wave's first row; row i has j = d0 - i
        if (d0 < -r || d0 > r + SDM_HZ_ROWS - 1) continue;              // (the same for the whole wave) no row of this wave is within r
        const f32x4 v = win[rr * SDM_HZ_TW + lane];
        const int k0 = d0 + r + (SDM_HZ_ROWS - 1);                      // 15 <= k0 <= 2 r + 30; k0 - i >= 0
#pragma unroll
        for (int i = 0; i < SDM_HZ_ROWS; ++i) hz_axpy(acc[i], wz[k0 - i], v);
      }
    }
  }

  float M[12] = {1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f};
  if (map) {
#pragma unroll
    for (int k = 0; k < 12; ++k) M[k] = map[b * 12 + k];
  } else if (map_id_out && y0 == 0 && x0 == 0 && tid < 12) {
    map_id_out[b * 12 + tid] = (tid == 0 || tid == 4 || tid == 8) ? 1.0f : 0.0f;
  }

  // Epilogue, a tile row (64 pixels = 192 consecutive floats) at a time: global <-> LDS as 3 x 64 consecutive dwords, LDS <-> registers as the lane's pixel
  // (dword index 3 lane + k: conflict-free).
  float* sF = strips[wv][0];
  float* sB = strips[wv][1];
  float* sO = strips[wv][2];
  float* sG = strips[wv][3];
  const int nfl = 3 * min(SDM_HZ_TW, W - x0);                           // floats of a tile row that exist
  const size_t bgoff = (size_t)(bg_batch == 1 ? 0 : b) * H;
#pragma unroll
  for (int i = 0; i < SDM_HZ_ROWS; ++i) {
    const int y = yw + i;
    if (y < H) {                                                        // (the same for the whole wave)
      const size_t g0 = ((size_t)b * H + y) * W + x0, gb = (bgoff + y) * W + x0;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const int j = lane + 64 * k;
        if (j < nfl) { sF[j] = fg[g0 * 3 + j]; sB[j] = bg[gb * 3 + j]; }
      }
      const float a = x < W ? gf_alpha(alpha[g0 + lane]) : 0.0f;
      SDM_WAVE_SYNC();
      if (x < W) {
        const float fr = sF[3 * lane], fgn = sF[3 * lane + 1], fb = sF[3 * lane + 2];
        const float m = acc[i][3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          float f = ((M[9 + k] + M[3 * k] * fr) + M[3 * k + 1] * fgn) + M[3 * k + 2] * fb;
          f = fminf(fmaxf(f, 0.0f), 1.0f);
          if (tplane) f = fminf(fmaxf(f + wrap * (acc[i][k] - m * f), 0.0f), 1.0f);
          sG[3 * lane + k] = f;
          sO[3 * lane + k] = a * f + (1.0f - a) * sB[3 * lane + k];
        }
      }
      SDM_WAVE_SYNC();
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const int j = lane + 64 * k;
        if (j < nfl) {
          out[g0 * 3 + j] = sO[j];
          if (fg_out) fg_out[g0 * 3 + j] = sG[j];
        }
      }
      SDM_WAVE_SYNC();                                                  // the strips are rewritten by the next row
    }
  }
}
