// k_distance.h - the exact Euclidean distance transform and its two consumers (sdm_distance_field / sdm_offset_mask / sdm_outline in
// include/sdmatte.h; DESIGN.md 4, "distance fields").
//
//   F = { p : plane[p] > threshold }                                  (one fp32 compare: NaN is outside F)
//   field[p] = +d2(p) for p in F, -d2(p) otherwise; d2(p) = min (dy^2 + dx^2) over the pixels of the OTHER class of the same image,
//   SDM_DF_FIELD_NONE where that class is empty.  Pixels beyond the border do not exist.  Integer arithmetic only, no radius cap.
//
// Four launches, whatever B, H, W and the content; the first three are the column pass, tiled in SDM_DF_TILE = 32 rows so that a tile of one column
// is ONE 32-bit word of class bits and a distance inside a tile is a count of leading / trailing zeros instead of a serial chain:
//   df_bits_kernel    plane -> one word per (tile, column): bit i = row 32 t + i is in F                       (reads 4 bytes, writes 1 bit per pixel)
//   df_carry_kernel   per column, down and up over the tile words: for every tile the row of the nearest pixel of F / outside F above it and
//                     below it.  One thread per column, H / 32 steps each way, every load independent of the chain (16 bytes per tile and column)
//   df_cols_kernel    per pixel the vertical distance to the nearest pixel of the other class in its column, from the tile word and the four
//                     carries: ONE unsigned 16-bit plane, bit 15 = the pixel's class, bits 0 .. 14 = the distance (1 .. 32767), 0 = the column
//                     holds no pixel of the other class
//   df_rows_kernel    per row the lower envelope of the parabolas (x - u)^2 + g(u)^2, exactly, by a pruned search: the row is staged in LDS as
//                     words [g to the nearest pixel outside F | g to the nearest pixel of F << 16] (0 for a column whose pixel in this row is of that
//                     class itself, SDM_DF_INF for none), with the minimum of either half per 64-column chunk beside it.  A wave owns the 64 pixels
//                     of one chunk and walks the chunks outwards; a chunk at least dxmin away with chunk minimum m cannot improve a pixel whose
//                     best is <= dxmin^2 + m^2, so it is read only if some lane of the wave can still gain from it (all 64 lanes then read the same
//                     LDS words: broadcasts), and the walk ends once the ring's nearest column is farther than every lane's best.  Both tests skip
//                     compares whose outcome is known.  An image that is all one class costs one chunk-minimum test per chunk; the search is long
//                     only where many chunks hold columns about as near as the best one (the inside of a large disk).
// The row pass writes the field (MODE 0) or applies a consumer's arithmetic to it in registers (MODE 1 sdm_offset_mask, MODE 2 sdm_outline): the
// consumers never store the field.
#pragma once
#include "sdm_common.h"

#define SDM_DF_TILE 32                   // rows of a column tile = bits of its class word
#define SDM_DF_CHUNK 64                  // columns of a chunk of the row pass = lanes of a wave
#define SDM_DF_INF 46340u                // "no such pixel" as a column distance: INF^2 = 2147395600 lies above every real d2 (<= 2 * 32767^2 = 2147352578),
                                         // and INF^2 + 32768^2 is still below 2^32, so that the search needs no 64-bit sum
#define SDM_DF_FIELD_NONE 0x7FFFFFFF     // = SDM_DF_NONE (include/sdmatte.h)
#define SDM_DF_NO_ROW_BELOW 0x7FFFFFFF   // df_carry_kernel: no such pixel below the tile (above: -1)

#ifdef SDM_EMU
#define SDM_DF_SQ(d) ((unsigned int)((d) * (d)))
#else
#define SDM_DF_SQ(d) ((unsigned int)__mul24((d), (d)))      // |d| < 2^15: the full-rate 24-bit multiply
#endif

// the rows of tile t that exist, as a bit mask
SDM_DEV_INLINE unsigned int df_tile_rows(int H, int t) {
  const int nv = min(SDM_DF_TILE, H - t * SDM_DF_TILE);
  return nv >= 32 ? 0xFFFFFFFFu : ((1u << nv) - 1u);
}

// grid: B * ceil(H / 32) * ceil(W / 256) blocks of 256 threads, one (tile, column) per thread: 32 independent loads, a wave reads 64 consecutive x
__global__ __launch_bounds__(256) void df_bits_kernel(const float* __restrict__ plane, unsigned int* __restrict__ bits, int B, int H, int W, float threshold) {
  const int nbx = (W + 255) / 256, nt = (H + SDM_DF_TILE - 1) / SDM_DF_TILE;
  const int blk = blockIdx.x;
  const int bx = blk % nbx, t = (blk / nbx) % nt, b = blk / (nbx * nt);
  const int x = bx * 256 + threadIdx.x;
  if (b >= B || x >= W) return;
  const int nv = min(SDM_DF_TILE, H - t * SDM_DF_TILE);
  const float* p = plane + ((size_t)b * H + (size_t)t * SDM_DF_TILE) * W + x;
  unsigned int m = 0u;
#pragma unroll
  for (int i = 0; i < SDM_DF_TILE; ++i)
    if (i < nv && p[(size_t)i * W] > threshold) m |= 1u << i;
  bits[((size_t)b * nt + t) * W + x] = m;
}

// grid: ceil(B * W / 256) blocks of 256 threads, one column per thread.  carry int32 [B][nt][4][W] = rows of {nearest F above, nearest non-F above,
// nearest F below, nearest non-F below} the tile (-1 / SDM_DF_NO_ROW_BELOW for none).
__global__ __launch_bounds__(256) void df_carry_kernel(const unsigned int* __restrict__ bits, int* __restrict__ carry, int B, int H, int W) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= B * W) return;
  const int b = i / W, x = i - b * W, nt = (H + SDM_DF_TILE - 1) / SDM_DF_TILE;
  const unsigned int* bp = bits + (size_t)b * nt * W + x;
  int* cp = carry + (size_t)b * nt * 4 * W + x;
  int rf = -1, rn = -1;
  for (int t = 0; t < nt; ++t) {
    const unsigned int vm = df_tile_rows(H, t), m = bp[(size_t)t * W], f = m & vm, n = ~m & vm;
    cp[((size_t)t * 4 + 0) * W] = rf;
    cp[((size_t)t * 4 + 1) * W] = rn;
    if (f) rf = t * SDM_DF_TILE + 31 - __builtin_clz(f);
    if (n) rn = t * SDM_DF_TILE + 31 - __builtin_clz(n);
  }
  rf = SDM_DF_NO_ROW_BELOW; rn = SDM_DF_NO_ROW_BELOW;
  for (int t = nt - 1; t >= 0; --t) {
    const unsigned int vm = df_tile_rows(H, t), m = bp[(size_t)t * W], f = m & vm, n = ~m & vm;
    cp[((size_t)t * 4 + 2) * W] = rf;
    cp[((size_t)t * 4 + 3) * W] = rn;
    if (f) rf = t * SDM_DF_TILE + __builtin_ctz(f);
    if (n) rn = t * SDM_DF_TILE + __builtin_ctz(n);
  }
}

// grid: as df_bits_kernel.  cols uint16 [B][H][W] (layout above).  The pixel's own bit is never one of the other class's, so "above" and "below" are
// the other class's bits on either side of it.
__global__ __launch_bounds__(256) void df_cols_kernel(const unsigned int* __restrict__ bits, const int* __restrict__ carry, unsigned short* __restrict__ cols,
                                                      int B, int H, int W) {
  const int nbx = (W + 255) / 256, nt = (H + SDM_DF_TILE - 1) / SDM_DF_TILE;
  const int blk = blockIdx.x;
  const int bx = blk % nbx, t = (blk / nbx) % nt, b = blk / (nbx * nt);
  const int x = bx * 256 + threadIdx.x;
  if (b >= B || x >= W) return;
  const int nv = min(SDM_DF_TILE, H - t * SDM_DF_TILE);
  const unsigned int vm = df_tile_rows(H, t), m = bits[((size_t)b * nt + t) * W + x], f = m & vm, n = ~m & vm;
  const int* cp = carry + ((size_t)b * nt + t) * 4 * W + x;
  const int up_f = cp[0], up_n = cp[W], dn_f = cp[(size_t)2 * W], dn_n = cp[(size_t)3 * W];
  unsigned short* dst = cols + ((size_t)b * H + (size_t)t * SDM_DF_TILE) * W + x;
#pragma unroll 4
  for (int i = 0; i < nv; ++i) {
    const int y = t * SDM_DF_TILE + i;
    const unsigned int c = (m >> i) & 1u;
    const unsigned int o = c ? n : f;
    const unsigned int above = o & ((1u << i) - 1u), below = (o >> i) >> 1;
    const int cu = c ? up_n : up_f, cd = c ? dn_n : dn_f;
    const int up = above ? i - (31 - __builtin_clz(above)) : (cu >= 0 ? y - cu : (int)SDM_DF_INF);
    const int dn = below ? __builtin_ctz(below) + 1 : (cd != SDM_DF_NO_ROW_BELOW ? cd - y : (int)SDM_DF_INF);
    const int d = min(up, dn);
    dst[(size_t)i * W] = (unsigned short)((d >= (int)SDM_DF_INF ? 0u : (unsigned int)d) | (c << 15));
  }
}

// what the row pass does with the field of a pixel
struct DfEmit {
  int32_t* field;                       // MODE 0
  float* out; float offset, feather;    // MODE 1: out = clamp((offset - sd) / feather + 0.5, 0, 1)
  // MODE 2: the stroke of sdm_outline around / over the straight-alpha cut-out (fg, alpha)
  const float* fg; const float* alpha; float* out_rgb; float* out_alpha;
  int position; float lo, hi, softness, opacity, rgb[3];
};

// signed distance in pixels with the silhouette half-way between the two classes: negative inside F, never in (-0.5, 0.5)
SDM_DEV_INLINE float df_signed_distance(int field) {
  const float r = sqrtf((float)(field < 0 ? -field : field)) - 0.5f;
  return field > 0 ? -r : r;
}

SDM_DEV_INLINE float df_ramp(float num, float den) { return fminf(fmaxf(num / den + 0.5f, 0.0f), 1.0f); }

template <int MODE>
SDM_DEV_INLINE void df_emit(const DfEmit& o, size_t i, int field) {
  if (MODE == 0) { o.field[i] = field; return; }
  const float sd = df_signed_distance(field);
  if (MODE == 1) { o.out[i] = df_ramp(o.offset - sd, o.feather); return; }
  // coverage of the band [lo, hi] (lo = -inf for position 0), stroke and subject as premultiplied layers, "over" in the order of the position
  float c = df_ramp(o.hi - sd, o.softness);
  if (o.position != 0) c *= df_ramp(sd - o.lo, o.softness);
  const float as = c * o.opacity;
  const float a = fminf(fmaxf(o.alpha[i], 0.0f), 1.0f);      // (NaN -> 0)
  // stroke under the subject (position 0) or over it: the stroke's share `ws` of the result's alpha A
  const float ws = o.position == 0 ? as * (1.0f - a) : as;
  const float A = o.position == 0 ? a + ws : as + a * (1.0f - as);
  // straight colour P / A as the subject's colour moved towards the stroke's by ws / A: exactly the subject's where the stroke adds nothing, and the
  // stroke's where there is no subject (whose colour means nothing there)
  const float t = A > 0.0f ? ws / A : 0.0f;
  for (int k = 0; k < 3; ++k) {
    const float f = o.fg[i * 3 + k], s = o.rgb[k];
    o.out_rgb[i * 3 + k] = A > 0.0f ? (a > 0.0f ? f + (s - f) * t : s) : 0.0f;
  }
  o.out_alpha[i] = A;
}

// dynamic LDS of df_rows_kernel: the row, padded to whole chunks, and one word of minima per chunk
SDM_HD_INLINE size_t df_rows_smem(int W) {
  const size_t nch = (size_t)((W + SDM_DF_CHUNK - 1) / SDM_DF_CHUNK);
  return nch * SDM_DF_CHUNK * 4 + nch * 4;
}

// one chunk of the search (wave-uniform call): `sh` selects the half of the words that holds the distances to the other class of this lane's pixel,
// dxmin is the lane's distance to the nearest column of chunk j
SDM_DEV_INLINE unsigned int df_scan_chunk(const unsigned int* row, const unsigned int* cmin, int j, int x, int sh, unsigned int dxmin, bool valid,
                                          unsigned int best) {
  const unsigned int cm = (cmin[j] >> sh) & 0xFFFFu;
  if (!__any((int)(valid && dxmin * dxmin + cm * cm < best))) return best;
  const u32x4* p = (const u32x4*)(row + j * SDM_DF_CHUNK);
  const int d0 = x - j * SDM_DF_CHUNK;      // x - u for the chunk's first column u
#pragma unroll 4
  for (int q = 0; q < SDM_DF_CHUNK / 4; ++q) {
    const u32x4 w = p[q];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const unsigned int g = (w[u] >> sh) & 0xFFFFu;
      const int d = d0 - (q * 4 + u);
      best = min(best, SDM_UMUL24(g, g) + SDM_DF_SQ(d));
    }
  }
  return best;
}

// grid: B * H blocks of 256 threads, one row per block; dynamic LDS df_rows_smem(W).  Wave w owns the pixels of chunks w, w + 4, ...
template <int MODE>
__global__ __launch_bounds__(256) void df_rows_kernel(const unsigned short* __restrict__ cols, int B, int H, int W, DfEmit o) {
  SDM_DYN_SMEM(smem);
  const int nch = (W + SDM_DF_CHUNK - 1) / SDM_DF_CHUNK;
  unsigned int* row = (unsigned int*)smem;                   // [nch * 64]
  unsigned int* cmin = row + (size_t)nch * SDM_DF_CHUNK;     // [nch]
  const size_t line = blockIdx.x;                            // = b * H + y
  if (line >= (size_t)B * H) return;
  const unsigned short* src = cols + line * W;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int j = wv; j < nch; j += 4) {
    const int x = j * SDM_DF_CHUNK + lane;
    unsigned int gn = SDM_DF_INF, gf = SDM_DF_INF;           // a column beyond the image: no pixel of either class
    if (x < W) {
      const unsigned int e = src[x];
      const unsigned int d = (e & 0x7FFFu) ? (e & 0x7FFFu) : SDM_DF_INF;
      if (e & 0x8000u) { gf = 0u; gn = d; } else { gn = 0u; gf = d; }
    }
    row[x] = gn | (gf << 16);
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
      gn = min(gn, (unsigned int)__shfl_xor((int)gn, s));
      gf = min(gf, (unsigned int)__shfl_xor((int)gf, s));
    }
    if (lane == 0) cmin[j] = gn | (gf << 16);
  }
  __syncthreads();
  for (int j0 = wv; j0 < nch; j0 += 4) {
    const int x = j0 * SDM_DF_CHUNK + lane;
    const bool valid = x < W;
    const unsigned int own = row[x];
    const bool fg = (own & 0xFFFFu) != 0u;                   // a pixel of F is at distance >= 1 from the pixels outside F
    const int sh = fg ? 0 : 16;
    const unsigned int g0 = (own >> sh) & 0xFFFFu;
    unsigned int best = g0 * g0;
    best = df_scan_chunk(row, cmin, j0, x, sh, 0u, valid, best);
    for (int k = 1; j0 - k >= 0 || j0 + k < nch; ++k) {
      const unsigned int dk = (unsigned int)(k - 1) * SDM_DF_CHUNK + 1u;      // the nearest column of ring k, seen from the wave's nearest lane
      if (!__any((int)(valid && dk * dk < best))) break;
      if (j0 - k >= 0) best = df_scan_chunk(row, cmin, j0 - k, x, sh, dk + (unsigned int)lane, valid, best);
      if (j0 + k < nch) best = df_scan_chunk(row, cmin, j0 + k, x, sh, dk + (unsigned int)(63 - lane), valid, best);
    }
    if (valid) {
      const int d2 = best >= SDM_DF_INF * SDM_DF_INF ? SDM_DF_FIELD_NONE : (int)best;
      df_emit<MODE>(o, line * W + x, fg ? d2 : -d2);
    }
  }
}
