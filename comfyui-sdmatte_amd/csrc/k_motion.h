// k_motion.h - the motion-compensated temporal filter of the alpha (sdm_smooth_alpha_motion; DESIGN.md 4, "motion-compensated temporal smoothing").
// sdm_smooth_alpha_temporal (k_temporal.h) with one change: a neighbouring frame is sampled along a block-matched integer displacement.
//
//   sanitise, clips, tau2, filter, limit: as k_temporal.h
//   candidates  for frames t and s = t + k of one clip, 0 < |k| <= radius, and pixel p: d = (dy, dx), |dy|, |dx| <= search, p + d inside the frame
//   distance    e_d(q) = (dr dr + dg dg) + db db of I_s(q + d) - I_t(q);  D_d(p) = (sum of e_d(q) over the q within Chebyshev distance `patch` of p for which
//               q and q + d both exist) / (3 n_d), n_d their number (a rectangle: rows x columns)
//   cost        C_d = D_d + pt (float)(dy dy + dx dx), pt = motion_penalty * tau2
//   choice      d* = the candidate with C_d == C_d and the smallest (C_d, dy dy + dx dx, dy, dx); none: the pair contributes nothing
//   weight      u = 1 - D_d* / tau2, u = u > 0 ? u : 0, w_k = (strength (1 - |k| / (radius + 1))) (u u); the sample is a_s(p + d*)
// True fp32 divisions, no contraction.  A zero weight adds +0 to both sums, an exact no-op.
//
// ONE launch per call: tsm_smooth_kernel<patch>; radius and search are runtime values.  It is a gather: the displacement differs per target pixel, so the pair
// symmetry and the register ring of ts_smooth_kernel do not carry over.  A block of 256 threads owns a tile of (64 - 2 patch) columns x 16 rows of ONE target
// frame and loops over that frame's neighbours in the order k = -1 .. -radius, +1 .. +radius.
//   * LDS holds one region of one frame at a time, a pixel as 16 bytes (r, g, b, sanitised alpha), pixels that do not exist as zeros: first the target's
//     (tile + `patch` halo), out of which every thread takes its column into registers, then each neighbour's (tile + `patch + search` halo: 80 x 36 pixels
//     = 45 KiB at the maxima, three blocks per CU).  Whether a pixel exists is decided from its coordinates, not from a mark.
//   * A wave is 64 consecutive COLUMNS of 4 rows (lane = column, `patch` halo lanes on either side), a thread owns the run of 4 pixels below each other in
//     its column.  So the 64 lanes of a 16-byte LDS read are 64 consecutive pixels for every displacement - conflict-free without any alignment of dx,
//     which a horizontal run cannot have.
//   * No barrier inside a neighbour.  Per displacement a thread forms e_d for the (4 + 2 patch) rows of its own column only (its target colours are in
//     registers), sums them down the column for its 4 pixels, and the sums of the 2 patch neighbouring columns come from the neighbouring lanes by wave
//     shuffles.  Every e_d(q) is formed (4 + 2 patch) / 4 * 64 / (64 - 2 patch) times (1.55 at patch 1), not (2 patch + 1)^2 times.
//   * Candidates are walked in the order (dy, dx) ascending, so "smaller cost, or equal cost and smaller dy dy + dx dx" keeps the lexicographic minimum.
//   * The loop over displacements is straight-line code: existence masks are ANDed into the bits of e, the choice is selects.
// The global loads are ts_load's: 3 x 16 bytes of image + 16 of alpha per aligned run of 4 pixels when W % 4 == 0 and the tensors are 16-byte aligned,
// scalar loads otherwise; the arithmetic behind them is one code path, so both give the same bits.  No load leaves the planes: a run is fetched only where
// its row and its first pixel lie in the frame, and only its pixels below W.
#pragma once
#include "sdm_common.h"
#include "k_guided.h"      // gf_alpha, gf_clamp01
#include "k_temporal.h"    // ts_load

#define SDM_TSM_TH 16                                                   // tile rows: 4 waves x 4
#define SDM_TSM_S 8                                                     // the largest search (SDM_TSM_MAX_SEARCH)
#define SDM_TSM_PITCH (64 + 2 * SDM_TSM_S)                              // region columns: the wave's 64 and `search` on either side

SDM_HD_INLINE int tsm_tile_w(int patch) { return 64 - 2 * patch; }

// the region [oy, oy + rh) x [ox, ox + rw) of frame f -> nb (row pitch SDM_TSM_PITCH); pixels outside the frame are written as zeros
SDM_DEV_INLINE void tsm_fill(f32x4* nb, const float* __restrict__ image, const float* __restrict__ alpha, int f, int H, int W, int oy, int ox, int rh, int rw,
                             bool vec) {
  const int xr0 = ox & ~3;                                              // (two's complement: rounds down for negative ox too)
  const int nruns = (((ox + rw - 1) & ~3) - xr0) / 4 + 1;
  for (int idx = threadIdx.x; idx < rh * nruns; idx += 256) {
    const int row = idx / nruns, xr = xr0 + (idx - row * nruns) * 4, y = oy + row;
    float c[12], a[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int i = 0; i < 12; ++i) c[i] = 0.0f;
    const int npx = (y >= 0 && y < H && xr >= 0 && xr < W) ? min(4, W - xr) : 0;
    if (npx > 0) ts_load(image, alpha, ((size_t)f * H + y) * W + xr, npx, vec, true, c, a);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int col = xr + i - ox;
      if (col >= 0 && col < rw) {
        f32x4 v;
        v[0] = c[3 * i]; v[1] = c[3 * i + 1]; v[2] = c[3 * i + 2]; v[3] = i < npx ? gf_alpha(a[i]) : 0.0f;
        nb[row * SDM_TSM_PITCH + col] = v;
      }
    }
  }
}

// grid: B * ceil(H / 16) * ceil(W / (64 - 2 P)) blocks of 256 threads.  vec: W % 4 == 0 and image, alpha 16-byte aligned.
template <int P>
__global__ __launch_bounds__(256) void tsm_smooth_kernel(const float* __restrict__ image, const float* __restrict__ alpha, int B, int H, int W, int L, int R,
                                                         int S, float tau2, float pt, float strength, float max_change, int vec,
                                                         float* __restrict__ out) {
#pragma clang fp contract(off)      // every product is rounded once: w is the same number in the numerator and in the denominator (a constant alpha stays put)
  constexpr int TW = 64 - 2 * P, WR = 4 + 2 * P;                        // tile columns; rows of a thread's window
  SDM_SHARED f32x4 nb[(SDM_TSM_TH + 2 * 2 + 2 * SDM_TSM_S) * SDM_TSM_PITCH];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int nbx = (W + TW - 1) / TW, nby = (H + SDM_TSM_TH - 1) / SDM_TSM_TH;
  const int blk = blockIdx.x;
  const int t = blk / (nbx * nby), y0 = ((blk / nbx) % nby) * SDM_TSM_TH, x0 = (blk % nbx) * TW;
  const int c0 = (t / L) * L, c1 = min(B, c0 + L);                      // the clip of frame t
  const int x = x0 - P + lane, y = y0 + 4 * wv;                         // this thread's column and the first of its 4 rows
  const bool col_in = x >= 0 && x < W;
  const bool owner = lane >= P && lane < 64 - P && col_in;              // this thread's pixels are output (those with y + i < H)
  const bool wide = vec != 0;

  // the target frame: the thread's column of the region (tile + patch halo), rows y - P .. y + 3 + P
  tsm_fill(nb, image, alpha, t, H, W, y0 - P, x0 - P, SDM_TSM_TH + 2 * P, 64, wide);
  __syncthreads();
  float tc[WR][3], at[4];
#pragma unroll
  for (int r = 0; r < WR; ++r) {
    const f32x4 v = nb[(4 * wv + r) * SDM_TSM_PITCH + lane];
    tc[r][0] = v[0]; tc[r][1] = v[1]; tc[r][2] = v[2];
    if (r >= P && r < P + 4) at[r - P] = v[3];
  }
  float num[4], den[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) { num[i] = at[i]; den[i] = 1.0f; }

  for (int kk = 0; kk < 2 * R; ++kk) {
    const int ka = kk < R ? kk + 1 : kk - R + 1;                       // |k|
    const int s = kk < R ? t - ka : t + ka;
    if (s < c0 || s >= c1) continue;                                    // (the same for the whole block)
    __syncthreads();                                                    // every read of the region's last content is behind us
    tsm_fill(nb, image, alpha, s, H, W, y0 - P - S, x0 - P - S, SDM_TSM_TH + 2 * P + 2 * S, 64 + 2 * S, wide);
    __syncthreads();
    // the best candidate so far per pixel; bdd == INT_MAX: none yet (a NaN cost fails both comparisons below, so it is never taken)
    float bC[4], bD[4], bA[4];
    int bdd[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) { bC[i] = __builtin_inff(); bD[i] = 0.0f; bA[i] = 0.0f; bdd[i] = 0x7fffffff; }
    for (int dy = -S; dy <= S; ++dy) {
      // Everything below is straight-line code on purpose: masks are ANDed into the bits of e (a select would be turned into a branch per row, with the
      // LDS reads waiting for each other behind it), and a masked term is +0 whatever the pixel held (NaN included).
      unsigned int rmask[WR];                                           // window row r: q and q + d both exist
#pragma unroll
      for (int r = 0; r < WR; ++r) { const int yq = y - P + r; rmask[r] = (yq >= 0 && yq < H && yq + dy >= 0 && yq + dy < H) ? 0xffffffffu : 0u; }
      float n3y[4];
      bool ey[4];                                                       // this thread's pixel i is output and p + d exists, as far as dy goes
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int yp = y + i;
        ey[i] = owner && yp < H && yp + dy >= 0 && yp + dy < H;
        n3y[i] = (float)(3 * (min(min(yp + P, H - 1), H - 1 - dy) - max(max(yp - P, 0), -dy) + 1));
      }
      const f32x4* nrow = nb + (4 * wv + S + dy) * SDM_TSM_PITCH + lane + S;
      for (int dx = -S; dx <= S; ++dx) {
        const bool cok = col_in && x + dx >= 0 && x + dx < W;           // this column: q and q + d both exist (for a pixel of it: p + d exists)
        const unsigned int cmask = cok ? 0xffffffffu : 0u;
        f32x4 n[WR];
#pragma unroll
        for (int r = 0; r < WR; ++r) n[r] = nrow[r * SDM_TSM_PITCH + dx];      // (inside the region for every lane and displacement)
        float e[WR];
#pragma unroll
        for (int r = 0; r < WR; ++r) {
          const float dr = n[r][0] - tc[r][0], dg = n[r][1] - tc[r][1], db = n[r][2] - tc[r][2];
          e[r] = __builtin_bit_cast(float, __builtin_bit_cast(unsigned int, (dr * dr + dg * dg) + db * db) & (rmask[r] & cmask));
        }
        float v[4], sum[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          v[i] = e[i];
#pragma unroll
          for (int r = 1; r <= 2 * P; ++r) v[i] += e[i + r];
          sum[i] = v[i];
        }
        if constexpr (P > 0) {                                          // the neighbouring columns' sums (every lane takes part; owners have all 2 P in the wave)
#pragma unroll
          for (int j = 1; j <= P; ++j) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              const float lo = __shfl(v[i], (lane - j) & 63), hi = __shfl(v[i], (lane + j) & 63);
              sum[i] += lo; sum[i] += hi;
            }
          }
        }
        const float nx = (float)(min(min(x + P, W - 1), W - 1 - dx) - max(max(x - P, 0), -dx) + 1);
        const int dd = dy * dy + dx * dx;
        const float pen = pt * (float)dd;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float D = sum[i] / (n3y[i] * nx);                       // (3 n_d: an integer below 2^24, exact; where the pixel is not eligible, anything)
          const float C = D + pen;
          const bool take = (ey[i] & cok) & ((C < bC[i]) | ((C == bC[i]) & (dd < bdd[i])));
          bC[i] = take ? C : bC[i]; bD[i] = take ? D : bD[i]; bA[i] = take ? n[P + i][3] : bA[i]; bdd[i] = take ? dd : bdd[i];
        }
      }
    }
    const float ck = strength * (1.0f - (float)ka / (float)(R + 1));
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (bdd[i] != 0x7fffffff) {
        float u = 1.0f - bD[i] / tau2;
        u = u > 0.0f ? u : 0.0f;
        const float w = ck * (u * u);
        num[i] += w * bA[i]; den[i] += w;
      }
    }
  }
  if (owner) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (y + i < H) {
        const float f = num[i] / den[i];
        const float d = fminf(fmaxf(f - at[i], -max_change), max_change);
        out[((size_t)t * H + y + i) * W + x] = gf_clamp01(at[i] + d);
      }
    }
  }
}
