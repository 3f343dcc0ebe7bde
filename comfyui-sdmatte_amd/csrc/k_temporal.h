// k_temporal.h - the image-guided temporal filter of the alpha (sdm_smooth_alpha_temporal; DESIGN.md 4, "temporal smoothing").  The batch axis is time.
//
//   sanitise  a = alpha with NaN -> 0, clamped to [0, 1]; image values as they are
//   clips     L = clip_len (B when 0); frames [i L, min(B, i L + L)) are clip i; clips are independent
//   distance  for frames t and s = t + k of one clip, 0 < |k| <= radius: e(q) = (dr dr + dg dg) + db db of I_s(q) - I_t(q);
//             D_k(p) = (sum of e over the existing pixels q within Chebyshev distance `patch` of p, row-major) / (3 n), n their number
//   weight    u = 1 - D_k(p) / tau2 (tau2 = color_tolerance * color_tolerance), u = u > 0 ? u : 0, g = u u, w_k = (strength (1 - |k| / (radius + 1))) g
//   filter    f = (a_t + sum_k w_k a_s) / (1 + sum_k w_k) over the k whose frame lies in the clip, in the order k = -1, -2, .., -radius, +1, +2, .., +radius
//   limit     out = clamp(a_t + clamp(f - a_t, -max_change, +max_change), 0, 1)
// True fp32 divisions.  A zero weight adds +0 to both sums, an exact no-op.
//
// ONE launch per call, whatever the arguments: ts_smooth_kernel<radius, patch>.  A block of 256 threads owns a tile of 64 columns x (14 - 2 patch) rows of
// one clip and walks the clip's frames in order.  A thread owns one run of 4 consecutive pixels of the tile's region (the tile plus a halo of `patch` rows
// above and below and of one run left and right: 18 runs x 14 rows = 252 threads):
//   * e needs the two frames at the SAME pixel only, so the colours of the last `radius` frames stay in the owner's registers (12 floats per frame), and
//     only e goes through LDS: when frame t arrives every thread writes e of the pairs (t, t - 1) .. (t, t - radius) for its run, one barrier, and the
//     threads of the tile's interior sum the patches (three 16-byte LDS reads per patch row serve 4 pixels).
//   * D is symmetric in (t, s): the pair's weight goes to both frames' sums, (numerator, denominator) of the last radius + 1 frames in registers.
//     Frame t - radius is then complete and is written.  Each frame is read once per tile that needs it (20 bytes per pixel and frame, plus the halo,
//     which the neighbouring tile's block fetches at about the same time), against 16 (2 radius + 1) + 4 for a gather.
//   * The ring is a register array indexed by compile-time indices only (the loops over `radius` are fully unrolled, the slots move by one per frame):
//     no scratch.  The next frame's loads are issued before the current frame is worked on.
//   * e is double-buffered in LDS (2 x radius x 14 x 72 floats: 32 KiB at radius 4, 16 KiB at radius 2), one barrier per frame.
// The loads are 3 x 16 bytes of image (+ 16 of alpha) per run when W % 4 == 0 and image, alpha and out are 16-byte aligned, 12 (+ 4) scalar loads otherwise;
// the arithmetic behind them is one code path, so both give the same bits.
#pragma once
#include "sdm_common.h"
#include "k_guided.h"      // gf_alpha, gf_clamp01

#define SDM_TS_TW 64                          // tile columns
#define SDM_TS_RC (SDM_TS_TW / 4 + 2)         // runs per region row: the tile's 16 and one of halo on either side
#define SDM_TS_RR 14                          // region rows: 14 x 18 = 252 runs
#define SDM_TS_RW (SDM_TS_RC * 4)             // region columns

SDM_HD_INLINE int ts_tile_h(int patch) { return SDM_TS_RR - 2 * patch; }

// the colours of a run (12 floats, pixel-major) and, for the tile's interior, its sanitised alpha; pixels i >= npx do not exist and read as 0
SDM_DEV_INLINE void ts_load(const float* __restrict__ image, const float* __restrict__ alpha, size_t g, int npx, bool vec, bool with_alpha, float (&c)[12],
                            float (&a)[4]) {
  if (vec) {
    const f32x4* ip = (const f32x4*)(image + g * 3);
    const f32x4 c0 = ip[0], c1 = ip[1], c2 = ip[2];
#pragma unroll
    for (int i = 0; i < 4; ++i) { c[i] = c0[i]; c[4 + i] = c1[i]; c[8 + i] = c2[i]; }
    if (with_alpha) {
      const f32x4 al = *(const f32x4*)(alpha + g);
#pragma unroll
      for (int i = 0; i < 4; ++i) a[i] = al[i];
    }
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      c[3 * i] = c[3 * i + 1] = c[3 * i + 2] = 0.0f;
      if (i < npx) {
        const float* ip = image + (g + i) * 3;
        c[3 * i] = ip[0]; c[3 * i + 1] = ip[1]; c[3 * i + 2] = ip[2];
        if (with_alpha) a[i] = alpha[g + i];
      }
    }
  }
}

// grid: ceil(B / L) * ceil(H / (14 - 2 P)) * ceil(W / 64) blocks of 256 threads.  vec: W % 4 == 0 and image, alpha, out 16-byte aligned.
template <int R, int P>
__global__ __launch_bounds__(256) void ts_smooth_kernel(const float* __restrict__ image, const float* __restrict__ alpha, int B, int H, int W, int L,
                                                        float tau2, float strength, float max_change, int vec, float* __restrict__ out) {
#pragma clang fp contract(off)      // every product is rounded once: w is the same number in the numerator and in the denominator (a constant alpha stays put)
  constexpr int TH = SDM_TS_RR - 2 * P;
  SDM_SHARED float es[2][R][SDM_TS_RR * SDM_TS_RW];
  const int tid = threadIdx.x;
  const int nbx = (W + SDM_TS_TW - 1) / SDM_TS_TW, nby = (H + TH - 1) / TH;
  const int blk = blockIdx.x;
  const int clip = blk / (nbx * nby), y0 = ((blk / nbx) % nby) * TH, x0 = (blk % nbx) * SDM_TS_TW;
  const int f0 = clip * L;
  if (f0 >= B) return;
  const int nf = min(L, B - f0);
  const int rr = tid / SDM_TS_RC, rc = tid % SDM_TS_RC;
  const int y = y0 - P + rr, x = x0 - 4 + rc * 4;                       // the first pixel of this thread's run
  const bool halo_run = rc == 0 || rc == SDM_TS_RC - 1;
  const bool have = rr < SDM_TS_RR && y >= 0 && y < H && x >= 0 && x < W && !(P == 0 && halo_run);
  const int npx = have ? min(4, W - x) : 0;
  const bool inner = have && !halo_run && rr >= P && rr < P + TH;      // this thread's run is output
  const bool wide = vec != 0;                                           // (then npx == 4 wherever `have`)
  const size_t frame_px = (size_t)H * W;
  const size_t g0 = (size_t)f0 * frame_px + (size_t)(have ? y : 0) * W + (have ? x : 0);
  const int li = rr * SDM_TS_RC + rc;                                   // this run's f32x4 index in a plane of es

  // what the patch sums of this run's pixels need, the same for every frame: the existing rows, the existing columns, 3 n
  const int ya = max(0, y - P), yb = min(H - 1, y + P);
  bool col_ok[4 + 2 * P];
#pragma unroll
  for (int j = 0; j < 4 + 2 * P; ++j) col_ok[j] = x - P + j >= 0 && x - P + j < W;
  float n3[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) n3[i] = (float)(3 * (yb - ya + 1) * (min(W - 1, x + i + P) - max(0, x + i - P) + 1));

  // ring slot k = frame (current - 1 - k): colours, alpha, numerator, denominator
  float pc[R][12], pa[R][4], pn[R][4], pd[R][4];
#pragma unroll
  for (int k = 0; k < R; ++k) {
#pragma unroll
    for (int i = 0; i < 12; ++i) pc[k][i] = 0.0f;
#pragma unroll
    for (int i = 0; i < 4; ++i) pa[k][i] = pn[k][i] = 0.0f, pd[k][i] = 1.0f;
  }
  float nc[12], na[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int i = 0; i < 12; ++i) nc[i] = 0.0f;
  if (have) ts_load(image, alpha, g0, npx, wide, inner, nc, na);

  auto emit = [&](const float (&a)[4], const float (&num)[4], const float (&den)[4], int frame) {
    float o[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float f = num[i] / den[i];
      const float d = fminf(fmaxf(f - a[i], -max_change), max_change);
      o[i] = gf_clamp01(a[i] + d);
    }
    float* op = out + g0 + (size_t)frame * frame_px;
    if (wide) {
      f32x4 v; v[0] = o[0]; v[1] = o[1]; v[2] = o[2]; v[3] = o[3];
      *(f32x4*)op = v;
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) if (i < npx) op[i] = o[i];
    }
  };

  for (int j = 0; j < nf; ++j) {
    float cc[12], ca[4], cn[4], cd[4];
#pragma unroll
    for (int i = 0; i < 12; ++i) cc[i] = nc[i];
#pragma unroll
    for (int i = 0; i < 4; ++i) { ca[i] = gf_alpha(na[i]); cn[i] = ca[i]; cd[i] = 1.0f; }
    if (have && j + 1 < nf) ts_load(image, alpha, g0 + (size_t)(j + 1) * frame_px, npx, wide, inner, nc, na);
    const int buf = j & 1;
    if (have) {
#pragma unroll
      for (int k = 0; k < R; ++k) {
        if (k < j) {
          f32x4 e;
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const float dr = cc[3 * i] - pc[k][3 * i], dg = cc[3 * i + 1] - pc[k][3 * i + 1], db = cc[3 * i + 2] - pc[k][3 * i + 2];
            e[i] = (dr * dr + dg * dg) + db * db;
          }
          ((f32x4*)es[buf][k])[li] = e;
        }
      }
    }
    __syncthreads();      // (the other buffer is written next: whoever writes it has passed this barrier, behind every read of two frames ago)
    if (inner) {
#pragma unroll
      for (int k = 0; k < R; ++k) {
        if (k < j) {
          float s[4] = {0.0f, 0.0f, 0.0f, 0.0f};
          for (int yy = ya; yy <= yb; ++yy) {
            const f32x4* er = (const f32x4*)es[buf][k] + (yy - (y0 - P)) * SDM_TS_RC + rc;
            float v[4 + 2 * P];
            const f32x4 m = er[0];
#pragma unroll
            for (int i = 0; i < 4; ++i) v[P + i] = m[i];
            if constexpr (P > 0) {
              const f32x4 l = er[-1], r = er[1];
#pragma unroll
              for (int i = 0; i < P; ++i) { v[i] = l[4 - P + i]; v[P + 4 + i] = r[i]; }
            }
#pragma unroll
            for (int i = 0; i < 4 + 2 * P; ++i) v[i] = col_ok[i] ? v[i] : 0.0f;      // (entries of pixels that do not exist were never written)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
#pragma unroll
              for (int dx = 0; dx <= 2 * P; ++dx) s[i] += v[i + dx];
            }
          }
          const float ck = strength * (1.0f - (float)(k + 1) / (float)(R + 1));
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            float u = 1.0f - (s[i] / n3[i]) / tau2;
            u = u > 0.0f ? u : 0.0f;
            const float w = ck * (u * u);
            cn[i] += w * pa[k][i]; cd[i] += w;
            pn[k][i] += w * ca[i]; pd[k][i] += w;
          }
        }
      }
      if (j >= R) emit(pa[R - 1], pn[R - 1], pd[R - 1], j - R);
    }
#pragma unroll
    for (int k = R - 1; k > 0; --k) {
#pragma unroll
      for (int i = 0; i < 12; ++i) pc[k][i] = pc[k - 1][i];
#pragma unroll
      for (int i = 0; i < 4; ++i) { pa[k][i] = pa[k - 1][i]; pn[k][i] = pn[k - 1][i]; pd[k][i] = pd[k - 1][i]; }
    }
#pragma unroll
    for (int i = 0; i < 12; ++i) pc[0][i] = cc[i];
#pragma unroll
    for (int i = 0; i < 4; ++i) { pa[0][i] = ca[i]; pn[0][i] = cn[i]; pd[0][i] = cd[i]; }
  }
  // the clip's last min(radius, nf) frames
  if (inner) {
#pragma unroll
    for (int k = R - 1; k >= 0; --k)
      if (k < nf) emit(pa[k], pn[k], pd[k], nf - 1 - k);
  }
}
