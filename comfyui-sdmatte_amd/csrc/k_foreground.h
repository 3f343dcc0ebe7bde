// k_foreground.h - multi-level foreground / background colour estimation from an image and its alpha (sdm_estimate_foreground; DESIGN.md 4,
// "foreground colours"), in the style of Germer et al., "Fast Multi-Level Foreground Estimation".
//
//   levels    (h_L, w_L) = (H, W), (h_{l-1}, w_{l-1}) = (ceil(h_l / 2), ceil(w_l / 2)) down to (1, 1); processed from (1, 1) upwards.
//             A level is SMALL iff max(h, w) <= 32: it runs n_small_iters Jacobi steps, every other level n_big_iters.
//   resample  nearest, integers only: src = min(Ns - 1, (i * Ns) / Nd).  I and a0 of a level come straight from the full-resolution inputs
//             (alpha sanitised: NaN -> 0, clamped to [0, 1]); F and B come from the previous level's result; at (1, 1) F = B = I.
//   weights   neighbours q = left, right, up, down with coordinates clamped to the level (a border pixel is its own neighbour):
//             w_q = regularization + gradient_weight * |a0[p] - a0[q]|,  s = sum w_q,  a1 = 1 - a0,  D = a0^2 + a1^2 + s
//   step      Fm = (sum w_q F[q]) / s, Bm = (sum w_q B[q]) / s, r = (I - a0 Fm - a1 Bm) / D,
//             F' = clamp(Fm + a0 r, 0, 1), B' = clamp(Bm + a1 r, 0, 1)            (the 2x2 solve with the a0 a1 terms cancelled on paper)
// Every step is a Jacobi step: it reads the previous step's values only, so the result does not depend on tiling, scheduling or batch position.
// True fp32 divisions (no reciprocal), subnormals kept: the GPU differs from another fp32 evaluation by FMA contraction and summation order only.
//
// Two kernels:
//   fg_small_kernel  one block of 1024 threads per image runs ALL small levels and all their steps: one thread per pixel (a small level has at most
//                    1024), a0 and two copies of F / B in LDS, the pixel's own I and weights in registers; one barrier per step.
//   fg_level_kernel  one launch per large level.  A block of 256 threads owns a 64 x 32 LDS region = a (64 - 2n) x (32 - 2n) tile plus a halo of
//                    n = n_big_iters pixels; it gathers I / a0 / F / B for the region, runs the n steps in LDS (the valid region shrinks by one
//                    ring per step) and stores the tile.
// Intermediate levels are planes of 8 floats per pixel [F.r F.g F.b B.r | B.g B.b 0 0]: two 16-byte loads or stores per pixel.
#pragma once
#include "sdm_common.h"

#define SDM_FG_SMALL 32          // a level is small iff max(h, w) <= SDM_FG_SMALL
#define SDM_FG_SMALL_PX 1024     // = SDM_FG_SMALL^2: threads of fg_small_kernel
#define SDM_FG_RW 64             // LDS region of an fg_level_kernel block: 64 x 32 pixels, tile + halo
#define SDM_FG_RH 32
#define SDM_FG_RPX (SDM_FG_RW * SDM_FG_RH)
#define SDM_FG_ROWS (SDM_FG_RH / 4)      // region rows per thread: wave v owns rows v, v + 4, ...

SDM_HD_INLINE int fg_tile_w(int n_big) { return SDM_FG_RW - 2 * n_big; }
SDM_HD_INLINE int fg_tile_h(int n_big) { return SDM_FG_RH - 2 * n_big; }

SDM_DEV_INLINE float fg_clamp01(float v) { return fminf(fmaxf(v, 0.0f), 1.0f); }
SDM_DEV_INLINE float fg_alpha(float a) { return fg_clamp01(a == a ? a : 0.0f); }

// one Jacobi step of one pixel.  nb[q][c]: F (c = 0..2) and B (c = 3..5) of neighbour q = left, right, up, down
SDM_DEV_INLINE void fg_step(const float (&I)[3], float a0, const float (&wq)[4], const float (&nb)[4][6], float (&out)[6]) {
  const float a1 = 1.0f - a0;
  const float s = ((wq[0] + wq[1]) + wq[2]) + wq[3];
  const float D = (a0 * a0 + a1 * a1) + s;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float Fm = (((wq[0] * nb[0][c] + wq[1] * nb[1][c]) + wq[2] * nb[2][c]) + wq[3] * nb[3][c]) / s;
    const float Bm = (((wq[0] * nb[0][c + 3] + wq[1] * nb[1][c + 3]) + wq[2] * nb[2][c + 3]) + wq[3] * nb[3][c + 3]) / s;
    const float r = ((I[c] - a0 * Fm) - a1 * Bm) / D;
    out[c] = fg_clamp01(Fm + a0 * r);
    out[c + 3] = fg_clamp01(Bm + a1 * r);
  }
}

// result of the top level, straight into the caller's tensors: fg [.., C] with the sanitised alpha as channel 3 when C = 4, bg [.., 3] unless NULL
SDM_DEV_INLINE void fg_store_top(float* __restrict__ fg, int C, float* __restrict__ bg, size_t pix, const float (&v)[6], float a0) {
  float* f = fg + pix * C;
  f[0] = v[0]; f[1] = v[1]; f[2] = v[2];
  if (C == 4) f[3] = a0;
  if (bg) { float* g = bg + pix * 3; g[0] = v[3]; g[1] = v[4]; g[2] = v[5]; }
}

SDM_DEV_INLINE void fg_store_plane(float* __restrict__ plane, size_t pix, const float (&v)[6]) {
  f32x4* p = (f32x4*)(plane + pix * 8);
  f32x4 lo, hi;
  lo[0] = v[0]; lo[1] = v[1]; lo[2] = v[2]; lo[3] = v[3];
  hi[0] = v[4]; hi[1] = v[5]; hi[2] = 0.0f; hi[3] = 0.0f;
  p[0] = lo; p[1] = hi;
}

// grid: B blocks of 1024 threads.  (hs, ws) = the largest small level, computed by the launcher with the rule above.  When (hs, ws) == (H, W) the
// result goes to fg / bg, otherwise to plane [B][hs * ws][8].
__global__ __launch_bounds__(SDM_FG_SMALL_PX) void fg_small_kernel(const float* __restrict__ image, const float* __restrict__ alpha, int B, int H, int W,
                                                                   int hs, int ws, float reg, float gw, int n_iters, float* __restrict__ plane,
                                                                   float* __restrict__ fg, int C, float* __restrict__ bg) {
  SDM_SHARED float sa[SDM_FG_SMALL_PX];
  SDM_SHARED float sv[2][6][SDM_FG_SMALL_PX];
  const int tid = threadIdx.x, b = blockIdx.x;
  if (b >= B) return;
  const float* img = image + (size_t)b * H * W * 3;
  const float* alp = alpha + (size_t)b * H * W;
  int nlev = 1;
  for (int h = hs, w = ws; h > 1 || w > 1; h = (h + 1) >> 1, w = (w + 1) >> 1) ++nlev;
  int cur = 0, ph = 1, pw = 1;
  for (int lv = nlev - 1; lv >= 0; --lv) {
    int h = hs, w = ws;
    for (int i = 0; i < lv; ++i) { h = (h + 1) >> 1; w = (w + 1) >> 1; }
    const bool act = tid < h * w;
    const int y = tid / w, x = tid - y * w;
    float I[3] = {0.0f, 0.0f, 0.0f}, a0 = 0.0f, v[6];
    if (act) {
      const int sy = min(H - 1, (y * H) / h), sx = min(W - 1, (x * W) / w);
      const size_t src = (size_t)sy * W + sx;
      I[0] = img[src * 3]; I[1] = img[src * 3 + 1]; I[2] = img[src * 3 + 2];
      a0 = fg_alpha(alp[src]);
      if (lv == nlev - 1) {
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = v[c + 3] = I[c];
      } else {
        const int p = min(ph - 1, (y * ph) / h) * pw + min(pw - 1, (x * pw) / w);
#pragma unroll
        for (int c = 0; c < 6; ++c) v[c] = sv[cur][c][p];
      }
    }
    __syncthreads();                       // the previous level has been read
    if (act) {
      sa[tid] = a0;
#pragma unroll
      for (int c = 0; c < 6; ++c) sv[cur][c][tid] = v[c];
    }
    __syncthreads();
    int q[4] = {tid, tid, tid, tid};
    float wq[4] = {reg, reg, reg, reg};
    if (act) {
      q[0] = x > 0 ? tid - 1 : tid; q[1] = x < w - 1 ? tid + 1 : tid; q[2] = y > 0 ? tid - w : tid; q[3] = y < h - 1 ? tid + w : tid;
#pragma unroll
      for (int k = 0; k < 4; ++k) wq[k] = reg + gw * fabsf(a0 - sa[q[k]]);
    }
    for (int it = 0; it < n_iters; ++it) {
      if (act) {
        float nb[4][6];
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
          for (int c = 0; c < 6; ++c) nb[k][c] = sv[cur][c][q[k]];
        fg_step(I, a0, wq, nb, v);
#pragma unroll
        for (int c = 0; c < 6; ++c) sv[cur ^ 1][c][tid] = v[c];
      }
      __syncthreads();
      cur ^= 1;
    }
    if (lv == 0 && act) {
      if (hs == H && ws == W) fg_store_top(fg, C, bg, (size_t)b * H * W + tid, v, a0);
      else fg_store_plane(plane, (size_t)b * hs * ws + tid, v);
    }
    ph = h; pw = w;
  }
}

// grid: B * ceil(h / tile_h) * ceil(w / tile_w) blocks of 256 threads; level (h, w), previous level prev [B][ph * pw][8] with (ph, pw) = (ceil(h / 2),
// ceil(w / 2)).  (h, w) == (H, W) is the top level: the tile goes to fg / bg, otherwise to plane [B][h * w][8].
// Thread t owns column t & 63 of region rows (t >> 6) + 4 j, j = 0 .. 7: a wave reads and writes whole LDS rows (no bank conflicts), and the pixel's I
// stays in registers.  A step computes into registers, then writes LDS behind a barrier, so one copy of F / B suffices (56 KB: two blocks per CU).
// With Nd = ceil(Ns' / 2) the resampling index (i * Nd) / Ns' of the F / B gather equals i >> 1 for every i < Ns' (even Ns': exact; odd Ns' = 2m - 1:
// i m / (2m - 1) = i / 2 + i / (2 (2m - 1)), and the second term never carries the floor over), so the gather needs no division.
__global__ __launch_bounds__(256) void fg_level_kernel(const float* __restrict__ image, const float* __restrict__ alpha, int B, int H, int W, int h, int w,
                                                       const float* __restrict__ prev, float reg, float gw, int n, float* __restrict__ plane,
                                                       float* __restrict__ fg, int C, float* __restrict__ bg) {
  SDM_SHARED float sa[SDM_FG_RPX];
  SDM_SHARED float sv[6][SDM_FG_RPX];
  const int tid = threadIdx.x;
  const int tw = fg_tile_w(n), th = fg_tile_h(n);
  const int nbx = (w + tw - 1) / tw, nby = (h + th - 1) / th;
  const int blk = blockIdx.x;
  const int b = blk / (nbx * nby), by = (blk / nbx) % nby, bx = blk % nbx;
  if (b >= B) return;
  const int pw = (w + 1) >> 1, ph = (h + 1) >> 1;
  const float* img = image + (size_t)b * H * W * 3;
  const float* alp = alpha + (size_t)b * H * W;
  const f32x4* pv = (const f32x4*)(prev + (size_t)b * ph * pw * 8);
  const int col = tid & 63, row0 = tid >> 6;
  const int x = bx * tw - n + col, y0 = by * th - n;
  const bool inx = x >= 0 && x < w;
  const int sx = inx ? (w == W ? x : min(W - 1, (x * W) / w)) : 0;
  float I[SDM_FG_ROWS][3], nv[SDM_FG_ROWS][6];
#pragma unroll
  for (int j = 0; j < SDM_FG_ROWS; ++j) {
    const int ry = row0 + 4 * j, y = y0 + ry, idx = ry * SDM_FG_RW + col;
    I[j][0] = I[j][1] = I[j][2] = 0.0f;
    if (inx && y >= 0 && y < h) {
      const int sy = h == H ? y : min(H - 1, (y * H) / h);
      const size_t src = (size_t)sy * W + sx;
      I[j][0] = img[src * 3]; I[j][1] = img[src * 3 + 1]; I[j][2] = img[src * 3 + 2];
      sa[idx] = fg_alpha(alp[src]);
      const size_t p = (size_t)(y >> 1) * pw + (x >> 1);
      const f32x4 lo = pv[p * 2], hi = pv[p * 2 + 1];
      sv[0][idx] = lo[0]; sv[1][idx] = lo[1]; sv[2][idx] = lo[2]; sv[3][idx] = lo[3]; sv[4][idx] = hi[0]; sv[5][idx] = hi[1];
    }
  }
  __syncthreads();
  for (int it = 1; it <= n; ++it) {
    // this step is valid `it` pixels inside the region (and inside the level)
    const bool cx = inx && col >= it && col < SDM_FG_RW - it;
#pragma unroll
    for (int j = 0; j < SDM_FG_ROWS; ++j) {
      const int ry = row0 + 4 * j, y = y0 + ry, idx = ry * SDM_FG_RW + col;
      if (cx && ry >= it && ry < SDM_FG_RH - it && y >= 0 && y < h) {
        const int q[4] = {x > 0 ? idx - 1 : idx, x < w - 1 ? idx + 1 : idx, y > 0 ? idx - SDM_FG_RW : idx, y < h - 1 ? idx + SDM_FG_RW : idx};
        const float a0 = sa[idx];
        float wq[4], nb[4][6];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          wq[k] = reg + gw * fabsf(a0 - sa[q[k]]);
#pragma unroll
          for (int c = 0; c < 6; ++c) nb[k][c] = sv[c][q[k]];
        }
        fg_step(I[j], a0, wq, nb, nv[j]);
      }
    }
    if (it == n) break;                    // the last step's values leave from the registers
    __syncthreads();
#pragma unroll
    for (int j = 0; j < SDM_FG_ROWS; ++j) {
      const int ry = row0 + 4 * j, y = y0 + ry, idx = ry * SDM_FG_RW + col;
      if (cx && ry >= it && ry < SDM_FG_RH - it && y >= 0 && y < h) {
#pragma unroll
        for (int c = 0; c < 6; ++c) sv[c][idx] = nv[j][c];
      }
    }
    __syncthreads();
  }
  const bool top = h == H && w == W;
  if (inx && col >= n && col < SDM_FG_RW - n) {
#pragma unroll
    for (int j = 0; j < SDM_FG_ROWS; ++j) {
      const int ry = row0 + 4 * j, y = y0 + ry, idx = ry * SDM_FG_RW + col;
      if (ry >= n && ry < SDM_FG_RH - n && y >= 0 && y < h) {
        const size_t pix = ((size_t)b * h + y) * w + x;
        if (top) fg_store_top(fg, C, bg, pix, nv[j], sa[idx]);
        else fg_store_plane(plane, pix, nv[j]);
      }
    }
  }
}
