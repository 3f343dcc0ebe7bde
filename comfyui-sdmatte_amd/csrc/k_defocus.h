// k_defocus.h - the subject over its own background out of focus (sdm_defocus_background; DESIGN.md 4, "background defocus").
//
//   a = clamp01(alpha, NaN -> 0);  C = bg or image;  F = fg or image
//   w(q)  = (1 - a(q)) * (1 + gain * max(0, (C.r + C.g + C.b) / 3 - threshold))
//   S(p)  = sum of w(q) C(q), N(p) = sum of w(q) over the closed disc dy dy + dx dx <= R R around p (pixels beyond the border do not exist)
//   Bb(p) = (S(p) + e C(p)) / (N(p) + e), e = 2^-10;  out(p) = a F(p) + (1 - a) Bb(p)
// fp32, true divisions, no contraction.
//
// A disc is (2 R + 1) row runs, and a row run is a difference of two prefix sums: 2 (2 R + 1) reads per pixel instead of about pi R R.  TWO launches:
//   dof_prefix_kernel  per row and per segment of 256 columns the segment-local inclusive prefix along x of (w C.r, w C.g, w C.b, w), 16 bytes per pixel, into
//                      an arena plane [B][H][W][4].  A wave owns one segment of one row: a thread its run of 4 pixels (ts_load: 3 x 16 + 16 bytes when the
//                      tensors are aligned and W % 4 == 0, scalar loads otherwise, one arithmetic path), summed in the thread, then the 64 thread totals are
//                      scanned with wave shuffles.  No LDS, no barrier.  Segment-local, not whole-row: a prefix stays below 256 (1 + gain), and so does what a
//                      difference cancels.  A segment's total is its last prefix value, so it needs no array of its own.
//   dof_gather_kernel  a block of 256 threads owns a tile of 64 x 64 output pixels: lane = column, a wave owns 16 rows and keeps their (S, N) in registers.
//                      The prefix rows y0 - R .. y0 + 63 + R go through LDS 8 at a time, columns x0 - R - 1 .. x0 + 63 + R (pixels that do not exist are
//                      written as zeros, so the prefix left of column 0 is 0 without a branch).  For a source row at distance dy the run of pixel x is
//                        P[min(x + hw, W - 1)] + (T - P[x - hw - 1]),  T = the left segment's total where the run crosses a segment boundary, else 0
//                      (at most one crossing: 2 R + 1 <= 129 < 256; with T = 0 this is P[..] - P[..] exactly).  Lanes are consecutive columns, so every 16-byte
//                      LDS read is conflict-free; the T read is made only by tiles whose window holds a segment boundary.  hw[] arrives by value and is kept one
//                      entry per lane, so a row's half width is a lane read, not a scalar load that the LDS reads would wait behind.  The rows
//                      of a disc are summed in ascending order: the order depends on the pixel's position only.  The epilogue adds the floor, divides and
//                      composes: Bb is never stored; colours and result cross a wave-private LDS strip so that global memory sees consecutive dwords.  N is clamped at 0 first: a sum of differences of rounded prefixes may come out a rounding error below
//                      0 where every weight is 0, and the denominator must stay >= e for `out == F where a == 1` to hold.
// No load leaves the planes: the window is fetched only where row and column lie in the image, every LDS index lies in the window (see the kernel), and the
// epilogue touches only pixels of the tile that exist.
#pragma once
#include "sdm_common.h"
#include "k_guided.h"      // gf_alpha
#include "k_temporal.h"    // ts_load

#define SDM_DOF_R 64                                                    // the largest radius (SDM_DEFOCUS_MAX_RADIUS)
#define SDM_DOF_SEG 256                                                 // columns of a prefix segment: 64 lanes x 4 pixels
#define SDM_DOF_TW 64                                                   // tile columns: a wave's lanes
#define SDM_DOF_TH 64                                                   // tile rows: 4 waves x 16
#define SDM_DOF_ROWS 16                                                 // output rows of a wave
#define SDM_DOF_CH 8                                                    // prefix rows in LDS at a time
#define SDM_DOF_PITCH (SDM_DOF_TW + 2 * SDM_DOF_R + 1)                  // window columns at the largest radius
#define SDM_DOF_FLOOR 0.0009765625f                                     // SDM_DEFOCUS_FLOOR = 2^-10

// the value of v in lane l, l the same for the whole wave (the emulator has shuffles only)
#ifdef SDM_EMU
#define SDM_DOF_READLANE(v, l) __shfl((v), (l))
#else
#define SDM_DOF_READLANE(v, l) __builtin_amdgcn_readlane((v), (l))
#endif

struct DofDisc { int r; unsigned char hw[SDM_DOF_R + 1]; };            // hw[|dy|]: the largest h with h h <= R R - dy dy (computed in integers on the host)

// grid: ceil(B * H * ceil(W / 256) / 4) blocks of 256 threads.  vec: W % 4 == 0 and C, alpha 16-byte aligned.
__global__ __launch_bounds__(256) void dof_prefix_kernel(const float* __restrict__ C, const float* __restrict__ alpha, int B, int H, int W, float gain,
                                                         float threshold, int vec, f32x4* __restrict__ plane) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int nseg = (W + SDM_DOF_SEG - 1) / SDM_DOF_SEG;
  const long long units = (long long)B * H * nseg, u = (long long)blockIdx.x * 4 + wv;
  const bool live = u < units;                                          // (a dead wave still takes part in its shuffles)
  const long long row = live ? u / nseg : 0;
  const int x = (live ? (int)(u - row * nseg) : 0) * SDM_DOF_SEG + lane * 4;
  const int npx = live ? max(0, min(4, W - x)) : 0;
  float c[12], a[4] = {1.0f, 1.0f, 1.0f, 1.0f};
#pragma unroll
  for (int i = 0; i < 12; ++i) c[i] = 0.0f;
  if (npx > 0) ts_load(C, alpha, (size_t)row * W + x, npx, vec != 0, true, c, a);
  f32x4 v[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float ai = gf_alpha(a[i]);
    const float Y = ((c[3 * i] + c[3 * i + 1]) + c[3 * i + 2]) / 3.0f;
    const float w = (1.0f - ai) * (1.0f + gain * fmaxf(0.0f, Y - threshold));
    v[i][0] = w * c[3 * i]; v[i][1] = w * c[3 * i + 1]; v[i][2] = w * c[3 * i + 2]; v[i][3] = w;
    if (i >= npx) v[i] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  }
  v[1] += v[0]; v[2] += v[1]; v[3] += v[2];                             // inclusive inside the thread's run
  f32x4 t = v[3];                                                       // ... and over the wave's 64 run totals
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float o = __shfl(t[k], (lane - d) & 63);
      if (lane >= d) t[k] += o;
    }
  }
  f32x4 ex;                                                             // what lies left of this thread's run in the segment
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float o = __shfl(t[k], (lane - 1) & 63);
    ex[k] = lane ? o : 0.0f;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (i < npx) plane[(size_t)row * W + x + i] = ex + v[i];
}

// grid: B * ceil(H / 64) * ceil(W / 64) blocks of 256 threads.
__global__ __launch_bounds__(256) void dof_gather_kernel(const f32x4* __restrict__ plane, const float* __restrict__ C, const float* __restrict__ F,
                                                         const float* __restrict__ alpha, int B, int H, int W, DofDisc disc, float* __restrict__ out) {
#pragma clang fp contract(off)
  SDM_SHARED f32x4 win[SDM_DOF_CH * SDM_DOF_PITCH];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int nbx = (W + SDM_DOF_TW - 1) / SDM_DOF_TW, nby = (H + SDM_DOF_TH - 1) / SDM_DOF_TH;
  const int blk = blockIdx.x;
  const int b = blk / (nbx * nby), y0 = ((blk / nbx) % nby) * SDM_DOF_TH, x0 = (blk % nbx) * SDM_DOF_TW;
  const int R = disc.r;
  const int wx0 = x0 - R - 1, ww = SDM_DOF_TW + 2 * R + 1;              // the window's first column (may be negative) and its width (<= SDM_DOF_PITCH)
  const int x = x0 + lane, xc = min(x, W - 1);                          // lanes right of the image work on its last column and store nothing; xc >= x0
  const int yw = y0 + SDM_DOF_ROWS * wv;                                // this wave's first output row
  const int hwv = lane <= R ? (int)disc.hw[lane] : 0;                   // lane l holds hw[l]: a row's half width is one lane read away, no scalar load
  // does the window hold a segment boundary?  (wx0 < 0 counts as one: harmless, T is then read from a zero column and not taken)
  const bool tile_cross = (wx0 >> 8) != (min(x0 + SDM_DOF_TW - 1 + R, W - 1) >> 8);
  f32x4 acc[SDM_DOF_ROWS];
#pragma unroll
  for (int i = 0; i < SDM_DOF_ROWS; ++i) acc[i] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

  const int r_lo = max(0, y0 - R), r_hi = min(H - 1, y0 + SDM_DOF_TH - 1 + R);
  for (int c0 = r_lo; c0 <= r_hi; c0 += SDM_DOF_CH) {
    const int nrows = min(SDM_DOF_CH, r_hi - c0 + 1);
    __syncthreads();                                                    // every read of the window's last content is behind us
    for (int idx = tid; idx < nrows * ww; idx += 256) {
      const int row = idx / ww, col = idx - row * ww, gx = wx0 + col;
      f32x4 v = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
      if (gx >= 0 && gx < W) v = plane[((size_t)b * H + c0 + row) * W + gx];      // (c0 + row lies in [0, H))
      win[row * SDM_DOF_PITCH + col] = v;
    }
    __syncthreads();
    for (int r = 0; r < nrows; ++r) {
      const int sr = c0 + r, base = r * SDM_DOF_PITCH - wx0;             // win[base + gx] is column gx of source row sr
      const int d0 = sr - yw;                                           // dy of the wave's first row; row i has dy = d0 - i
      // one row run: window columns xr <= x0 + 63 + R = wx0 + ww - 1 and xl >= x0 - R - 1 = wx0 (xl < 0: a zero column).  hw[R] is 0 for every R, and
      // lane 64 does not exist.  bx is the first column of xr's segment: the run crosses into it iff xl < bx; bx - 1 <= xr, and where xl < bx also
      // bx - 1 >= xl >= wx0.
#define SDM_DOF_RUN(i)                                                                         \
  {                                                                                            \
    const int dy = d0 - (i), ady = dy < 0 ? -dy : dy;                                          \
    const int h = ady == R ? 0 : SDM_DOF_READLANE(hwv, ady);                                   \
    const int xr = min(xc + h, W - 1), xl = xc - h - 1;                                        \
    const f32x4 A = win[base + xr], Bv = win[base + xl];                                       \
    f32x4 Tv = f32x4{0.0f, 0.0f, 0.0f, 0.0f};                                                  \
    if (tile_cross) {                                                                          \
      const int bx = xr & ~(SDM_DOF_SEG - 1);                                                  \
      const f32x4 tl = win[base + max(bx - 1, wx0)];                                           \
      if (xl < bx) Tv = tl;                                                                    \
    }                                                                                          \
    acc[i] += A + (Tv - Bv);                                                                   \
  }
#pragma unroll
      for (int i = 0; i < SDM_DOF_ROWS; ++i) {
        const int dyi = d0 - i;
        if (dyi <= R && dyi >= -R) SDM_DOF_RUN(i)                        // (the same for the whole wave)
      }
#undef SDM_DOF_RUN
    }
  }

  // Epilogue, a tile row (64 pixels = 192 consecutive floats) at a time.  A lane's own pixel is 3 floats at a stride of 12 bytes, which as global loads and
  // stores touches every cache line three times with a third of it; so the colours cross a wave-private strip of the (now idle) window: global <-> LDS as
  // 3 x 64 consecutive dwords, LDS <-> registers as the lane's pixel (dword index 3 lane + k: 3 is coprime to the bank count, conflict-free).  Dword
  // accesses only, so there is one path for every alignment.
  __syncthreads();                                                      // every read of the window is behind us
  float* sC = (float*)win + wv * (3 * 3 * SDM_DOF_TW);                  // this wave's strips: C, F, out
  float* sF = sC + 3 * SDM_DOF_TW;
  float* sO = sF + 3 * SDM_DOF_TW;
  const bool planes = F != C;                                           // (uniform)
  const int nfl = 3 * min(SDM_DOF_TW, W - x0);                          // floats of a tile row that exist
#pragma unroll
  for (int i = 0; i < SDM_DOF_ROWS; ++i) {
    const int y = yw + i;
    if (y < H) {                                                        // (the same for the whole wave)
      const size_t g0 = ((size_t)b * H + y) * W + x0;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const int j = lane + 64 * k;
        if (j < nfl) {
          sC[j] = C[g0 * 3 + j];
          if (planes) sF[j] = F[g0 * 3 + j];
        }
      }
      const float a = x < W ? gf_alpha(alpha[g0 + lane]) : 0.0f;
      SDM_WAVE_SYNC();
      if (x < W) {
        const float den = fmaxf(acc[i][3], 0.0f) + SDM_DOF_FLOOR;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const float c = sC[3 * lane + k], f = planes ? sF[3 * lane + k] : c;
          const float bb = (acc[i][k] + SDM_DOF_FLOOR * c) / den;
          sO[3 * lane + k] = a * f + (1.0f - a) * bb;
        }
      }
      SDM_WAVE_SYNC();
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const int j = lane + 64 * k;
        if (j < nfl) out[g0 * 3 + j] = sO[j];
      }
      SDM_WAVE_SYNC();                                                  // the strips are rewritten by the next row
    }
  }
}
