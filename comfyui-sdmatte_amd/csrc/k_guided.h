// k_guided.h - alpha refinement at the caller's resolution by the subsampled colour guided filter (sdm_refine_alpha_guided; DESIGN.md 4, "guided
// upsampling"): He, Sun, Tang, "Guided Image Filtering"; He, Sun, "Fast Guided Filter".
//
//   sanitise  p = alpha with NaN -> 0, clamped to [0, 1]; image values as they are
//   coarse    (h, w) = (ceil(H / s), ceil(W / s)); I' (3 channels) and p' of coarse pixel (i, j) = mean over the existing pixels of block
//             [i s, min(H, i s + s)) x [j s, min(W, j s + s)): the sum in row-major order, divided by the count
//   window    Win(i, j) = coarse pixels within Chebyshev distance `radius`, clipped to the grid, n of them; m(x) = (sum over Win) / n, the sum taken
//             along x first (ascending), then along y (ascending)
//   moments   mu = m(I'), mup = m(p'), c = m(I' p') - mu mup, Sigma = m(I' I'^T) - mu mu^T + eps Id   (13 window sums: 3 + 1 + 3 + 6)
//   solve     a = adj(Sigma) c / det(Sigma) (closed form of the symmetric 3 x 3), b = mup - a . mu
//   smooth    abar = m(a), bbar = m(b)
//   upsample  u = clamp((y + 0.5) / s - 0.5, 0, h - 1), i0 = floor(u), i1 = min(i0 + 1, h - 1), fy = u - i0, likewise j0, j1, fx along x;
//             v(j) = (1 - fy) v[i0][j] + fy v[i1][j], v^ = (1 - fx) v(j0) + fx v(j1)
//   apply     out = clamp(abar^ . I + bbar^, 0, 1)
// True fp32 divisions, direct window sums in a fixed order (no running prefix sums): an image's result depends neither on the tiling nor on the batch it is in.
//
// FOUR launches per call, whatever B, H, W, s and radius; the batch is part of every grid:
//   gf_mean_kernel    full resolution -> coarse plane [B][h][w][4] = (I'.r, I'.g, I'.b, p').  Reads image and alpha once (16 B / pixel).  One thread per
//                     coarse pixel (per 4 / s of them for s = 1, 2) walks its block in runs of 4 pixels = 3 x 16 B of image + 16 B of alpha when W % 4 == 0
//                     and s is 1, 2 or a multiple of 4; pixel by pixel otherwise, with the same order of additions.
//   gf_box_kernel<1>  coarse plane -> (a, b) plane [B][h][w][4].  A block of 256 threads owns a tile of 16 columns x gf_tile_h(radius) rows: it forms the
//                     13 products while it sums along x (2 radius + 1 neighbours straight from the plane, which is L2 / L1 resident: every 16-byte entry
//                     serves 13 sums) for the tile's rows plus a halo of `radius` rows, keeps these row sums in LDS (13 planes of 72 x 16 floats), sums them
//                     along y out of LDS and solves.  The moment planes never exist in memory.
//   gf_box_kernel<0>  (a, b) plane -> (abar, bbar) plane, the same kernel with 4 sums and no solve.
//   gf_apply_kernel   full resolution: reads the image once, writes the output once (16 B / pixel).  One thread per run of 4 consecutive pixels of the flat
//                     [B H W] index (3 x 16 B in, 16 B out, whatever W is); the coarse entries come through L1 / L2, and a thread keeps the vertically
//                     interpolated columns j0, j1 in registers from one pixel to the next.
// With s > 1 these are exactly two full-resolution passes and no full-resolution plane in the arena; with s = 1 the coarse grid is the image.
#pragma once
#include "sdm_common.h"

#define SDM_GF_TW 16             // tile columns of gf_box_kernel
#define SDM_GF_RR 72             // LDS rows: tile rows + 2 radius (SDM_GF_MAX_RADIUS = 32 leaves 8 tile rows)
#define SDM_GF_TH 24             // tile rows at radius <= 24
#define SDM_GF_NM 13             // window sums of the fit: I' (3), p', I' p' (3), I' I'^T (6)

SDM_HD_INLINE int gf_tile_h(int radius) { return SDM_GF_RR - 2 * radius < SDM_GF_TH ? SDM_GF_RR - 2 * radius : SDM_GF_TH; }

SDM_DEV_INLINE float gf_clamp01(float v) { return fminf(fmaxf(v, 0.0f), 1.0f); }
SDM_DEV_INLINE float gf_alpha(float a) { return gf_clamp01(a == a ? a : 0.0f); }

// grid: ceil(B * h * (w / G) / 256) blocks of 256 threads; thread -> (image, coarse row, group of G coarse pixels).  VEC needs W % 4 == 0, 16-byte aligned
// tensors and G * s a multiple of 4 (G = 4 / s for s = 1, 2; G = 1 for s = 4, 8, 12, 16); then w % G == 0 and every run of 4 pixels is aligned.
template <int G, bool VEC>
__global__ __launch_bounds__(256) void gf_mean_kernel(const float* __restrict__ image, const float* __restrict__ alpha, int B, int H, int W, int s, int h,
                                                      int w, float* __restrict__ coarse) {
  const int wg = w / G;
  const int t = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (t >= B * h * wg) return;
  const int jg = t % wg, i = (t / wg) % h, b = t / (wg * h);
  const int ya = i * s, yb = min(H, ya + s);
  const int xa = jg * G * s, xb = min(W, xa + G * s);
  float acc[G][4];
#pragma unroll
  for (int g = 0; g < G; ++g) acc[g][0] = acc[g][1] = acc[g][2] = acc[g][3] = 0.0f;
  for (int y = ya; y < yb; ++y) {
    const size_t row = ((size_t)b * H + y) * W;
    if (VEC) {
      for (int x = xa; x < xb; x += 4) {
        const f32x4* ip = (const f32x4*)(image + (row + x) * 3);
        const f32x4 c0 = ip[0], c1 = ip[1], c2 = ip[2];
        const f32x4 al = *(const f32x4*)(alpha + row + x);
        const float px[4][4] = {{c0[0], c0[1], c0[2], al[0]}, {c0[3], c1[0], c1[1], al[1]}, {c1[2], c1[3], c2[0], al[2]}, {c2[1], c2[2], c2[3], al[3]}};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int g = G == 4 ? k : (G == 2 ? k >> 1 : 0);      // with G > 1 the group is one run: pixel k belongs to coarse pixel k / s
          acc[g][0] += px[k][0]; acc[g][1] += px[k][1]; acc[g][2] += px[k][2]; acc[g][3] += gf_alpha(px[k][3]);
        }
      }
    } else {
      for (int x = xa; x < xb; ++x) {
        const float* ip = image + (row + x) * 3;
        acc[0][0] += ip[0]; acc[0][1] += ip[1]; acc[0][2] += ip[2]; acc[0][3] += gf_alpha(alpha[row + x]);
      }
    }
  }
  f32x4* dst = (f32x4*)coarse + ((size_t)b * h + i) * w + (size_t)jg * G;
#pragma unroll
  for (int g = 0; g < G; ++g) {
    const int ga = xa + g * s, gb = min(W, ga + s);
    const float n = (float)((yb - ya) * (gb - ga));
    f32x4 v;
    v[0] = acc[g][0] / n; v[1] = acc[g][1] / n; v[2] = acc[g][2] / n; v[3] = acc[g][3] / n;
    dst[g] = v;
  }
}

// a = adj(Sigma) c / det(Sigma), b = mup - a . mu from the 13 window means m[] (order: SDM_GF_NM above)
SDM_DEV_INLINE f32x4 gf_solve(const float (&m)[SDM_GF_NM], float eps) {
  const float c0 = m[4] - m[0] * m[3], c1 = m[5] - m[1] * m[3], c2 = m[6] - m[2] * m[3];
  const float s00 = (m[7] - m[0] * m[0]) + eps, s01 = m[8] - m[0] * m[1], s02 = m[9] - m[0] * m[2];
  const float s11 = (m[10] - m[1] * m[1]) + eps, s12 = m[11] - m[1] * m[2], s22 = (m[12] - m[2] * m[2]) + eps;
  const float k00 = s11 * s22 - s12 * s12, k01 = s02 * s12 - s01 * s22, k02 = s01 * s12 - s02 * s11;
  const float k11 = s00 * s22 - s02 * s02, k12 = s01 * s02 - s00 * s12, k22 = s00 * s11 - s01 * s01;
  const float det = (s00 * k00 + s01 * k01) + s02 * k02;
  f32x4 r;
  r[0] = ((k00 * c0 + k01 * c1) + k02 * c2) / det;
  r[1] = ((k01 * c0 + k11 * c1) + k12 * c2) / det;
  r[2] = ((k02 * c0 + k12 * c1) + k22 * c2) / det;
  r[3] = m[3] - ((r[0] * m[0] + r[1] * m[1]) + r[2] * m[2]);
  return r;
}

// grid: B * ceil(h / gf_tile_h(radius)) * ceil(w / 16) blocks of 256 threads.  src, dst: planes [B][h][w][4].  FIT: src = (I', p'), dst = (a, b);
// otherwise dst = the window mean of src.  LDS entry (region row rr, column col) of sum k is hs[k][rr * 16 + col]: the lanes of a wave read and write
// consecutive floats.  Entries of rows or columns beyond the grid are neither written nor read.
template <bool FIT>
__global__ __launch_bounds__(256) void gf_box_kernel(const float* __restrict__ src, int B, int h, int w, int radius, float eps, float* __restrict__ dst) {
  constexpr int NM = FIT ? SDM_GF_NM : 4;
  SDM_SHARED float hs[NM][SDM_GF_RR * SDM_GF_TW];
  const int tid = threadIdx.x;
  const int th = gf_tile_h(radius);
  const int nbx = (w + SDM_GF_TW - 1) / SDM_GF_TW, nby = (h + th - 1) / th;
  const int blk = blockIdx.x;
  const int b = blk / (nbx * nby), y0 = ((blk / nbx) % nby) * th, x0 = (blk % nbx) * SDM_GF_TW;
  if (b >= B) return;
  const f32x4* sp = (const f32x4*)src + (size_t)b * h * w;
  for (int idx = tid; idx < (th + 2 * radius) * SDM_GF_TW; idx += 256) {
    const int y = y0 - radius + (idx >> 4), x = x0 + (idx & 15);
    if (y >= 0 && y < h && x < w) {
      const f32x4* rowp = sp + (size_t)y * w;
      const int xb = min(w - 1, x + radius);
      float m[NM];
#pragma unroll
      for (int k = 0; k < NM; ++k) m[k] = 0.0f;
#pragma unroll 4
      for (int xx = max(0, x - radius); xx <= xb; ++xx) {
        const f32x4 v = rowp[xx];
        m[0] += v[0]; m[1] += v[1]; m[2] += v[2]; m[3] += v[3];
        if constexpr (FIT) {
          m[4] += v[0] * v[3]; m[5] += v[1] * v[3]; m[6] += v[2] * v[3];
          m[7] += v[0] * v[0]; m[8] += v[0] * v[1]; m[9] += v[0] * v[2]; m[10] += v[1] * v[1]; m[11] += v[1] * v[2]; m[12] += v[2] * v[2];
        }
      }
#pragma unroll
      for (int k = 0; k < NM; ++k) hs[k][idx] = m[k];
    }
  }
  __syncthreads();
  for (int idx = tid; idx < th * SDM_GF_TW; idx += 256) {
    const int y = y0 + (idx >> 4), col = idx & 15, x = x0 + col;
    if (y < h && x < w) {
      const int ya = max(0, y - radius), yb = min(h - 1, y + radius);
      float m[NM];
#pragma unroll
      for (int k = 0; k < NM; ++k) m[k] = 0.0f;
      for (int yy = ya; yy <= yb; ++yy) {
        const int li = (yy - y0 + radius) * SDM_GF_TW + col;
#pragma unroll
        for (int k = 0; k < NM; ++k) m[k] += hs[k][li];
      }
      const float n = (float)((yb - ya + 1) * (min(w - 1, x + radius) - max(0, x - radius) + 1));
#pragma unroll
      for (int k = 0; k < NM; ++k) m[k] = m[k] / n;
      f32x4 r;
      if constexpr (FIT) {
        r = gf_solve(m, eps);
      } else {
        r[0] = m[0]; r[1] = m[1]; r[2] = m[2]; r[3] = m[3];
      }
      ((f32x4*)dst)[((size_t)b * h + y) * w + x] = r;
    }
  }
}

// (1 - fy) v[i0][j] + fy v[i1][j] of the (abar, bbar) plane of one image
SDM_DEV_INLINE f32x4 gf_vlerp(const f32x4* __restrict__ ab, int w, int i0, int i1, float fy, int j) {
  const f32x4 t = ab[(size_t)i0 * w + j], u = ab[(size_t)i1 * w + j];
  const float gy = 1.0f - fy;
  f32x4 r;
  r[0] = gy * t[0] + fy * u[0]; r[1] = gy * t[1] + fy * u[1]; r[2] = gy * t[2] + fy * u[2]; r[3] = gy * t[3] + fy * u[3];
  return r;
}

// source coordinate of full-resolution index i on a coarse axis of n entries: u = clamp((i + 0.5) / s - 0.5, 0, n - 1) -> i0 = floor(u), frac = u - i0
SDM_DEV_INLINE void gf_coord(int i, float fs, int n, int& i0, int& i1, float& frac) {
  const float u = fminf(fmaxf(((float)i + 0.5f) / fs - 0.5f, 0.0f), (float)(n - 1));
  i0 = (int)u; i1 = min(i0 + 1, n - 1); frac = u - (float)i0;
}

// grid: ceil(ceil(B * H * W / 4) / 256) blocks of 256 threads; thread -> pixels 4 t .. 4 t + 3 of the flat [B H W] index (a run may cross the end of a row
// or of an image).  vec: image and out are 16-byte aligned; the last run of a tensor whose pixel count is no multiple of 4 goes pixel by pixel.
__global__ __launch_bounds__(256) void gf_apply_kernel(const float* __restrict__ image, const float* __restrict__ ab, int B, int H, int W, int s, int h, int w,
                                                       int vec, float* __restrict__ out) {
  const int total = B * H * W;
  const int t = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (t >= (total + 3) / 4) return;
  const int g0 = t * 4, n = min(4, total - g0);
  const bool wide = vec && n == 4;
  float I[4][3];
  if (wide) {
    const f32x4* ip = (const f32x4*)(image + (size_t)g0 * 3);
    const f32x4 c0 = ip[0], c1 = ip[1], c2 = ip[2];
    I[0][0] = c0[0]; I[0][1] = c0[1]; I[0][2] = c0[2]; I[1][0] = c0[3]; I[1][1] = c1[0]; I[1][2] = c1[1];
    I[2][0] = c1[2]; I[2][1] = c1[3]; I[2][2] = c2[0]; I[3][0] = c2[1]; I[3][1] = c2[2]; I[3][2] = c2[3];
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      I[k][0] = I[k][1] = I[k][2] = 0.0f;
      if (k < n) { const float* ip = image + (size_t)(g0 + k) * 3; I[k][0] = ip[0]; I[k][1] = ip[1]; I[k][2] = ip[2]; }
    }
  }
  int x = g0 % W, y = (g0 / W) % H, b = g0 / (W * H);
  const float fs = (float)s;
  float res[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  const f32x4* abp = nullptr;
  int i0 = 0, i1 = 0, cj = -2;
  float fy = 0.0f;
  f32x4 cl = {0.0f, 0.0f, 0.0f, 0.0f}, cr = cl;      // the vertically interpolated columns cj and min(cj + 1, w - 1)
  bool new_row = true;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (k < n) {
      if (new_row) {
        gf_coord(y, fs, h, i0, i1, fy);
        abp = (const f32x4*)ab + (size_t)b * h * w;
        cj = -2; new_row = false;
      }
      int j0, j1; float fx;
      gf_coord(x, fs, w, j0, j1, fx);
      if (j0 != cj) {
        cl = j0 == cj + 1 ? cr : gf_vlerp(abp, w, i0, i1, fy, j0);      // (cj + 1 <= w - 1 here, so cr is column cj + 1)
        cr = j1 == j0 ? cl : gf_vlerp(abp, w, i0, i1, fy, j1);
        cj = j0;
      }
      const float gx = 1.0f - fx;
      const float a0 = gx * cl[0] + fx * cr[0], a1 = gx * cl[1] + fx * cr[1], a2 = gx * cl[2] + fx * cr[2], bb = gx * cl[3] + fx * cr[3];
      res[k] = gf_clamp01(((a0 * I[k][0] + a1 * I[k][1]) + a2 * I[k][2]) + bb);
      if (++x == W) { x = 0; new_row = true; if (++y == H) { y = 0; ++b; } }
    }
  }
  if (wide) {
    f32x4 o; o[0] = res[0]; o[1] = res[1]; o[2] = res[2]; o[3] = res[3];
    *(f32x4*)(out + g0) = o;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) if (k < n) out[g0 + k] = res[k];
  }
}
