// k_tiles.h - tiles along the trimap's unknown band and the node call that blends them (sdm_band_tiles / sdm_apply_matte_tiles in include/sdmatte.h;
// DESIGN.md 4, "matte at the photo's own resolution").
//
// sdm_band_tiles: the grid of an axis of length L is {n, d, size} (TilesAxis): n tiles of `size` pixels at the origins o_i = (i * d) / (n - 1), d = L - T
// (one tile of L pixels at 0 if L <= T).  The origins increase, so the tiles that contain a coordinate are a contiguous range [lo, hi] of indices.
//   tiles_init_kernel   flag words = 0: SDM_TL_WORDS words per image, bit iy * n_x + ix of them is grid cell (iy, ix)
//   tiles_mark_kernel   one read of the plane, roi_reduce_kernel's layout and load paths.  The origin tables of both axes sit in LDS; a wave without a
//                       band pixel (wave vote) goes on to its next load; a band pixel (on the vector path: the band pixels of a vector, whose ranges
//                       join to one, see tiles_mark_span) ORs its cells into the block's bitmask in LDS; then at most one global atomicOr per non-zero
//                       word and block.  No global atomic per pixel.
//   tiles_list_kernel   one thread per image: the set cells in row-major order as entries {b, y0, x0, h, w}, the void entries, the count
// Three launches, whatever B, H, W and the content; integer and bitwise operations only.
//
// sdm_apply_matte_tiles: boxes_sanitize_kernel, boxes_prep_image_kernel, boxes_prep_trimap_kernel (k_boxes.h) and the model as in sdm_apply_matte_boxes;
// tiles_blend_kernel writes every frame pixel once: the weighted mean, with weights that ramp down towards a tile's inner edges, of roi_paste_kernel's
// value over the valid tiles that contain it, the base where there is none.
#pragma once
#include "sdm_common.h"
#include "k_boxes.h"

#define SDM_TL_WORDS 8               // flag words per image: SDM_TILES_MAX_GRID / 32
#define SDM_TL_AXIS 256              // tiles per axis at most (n_y * n_x <= SDM_TILES_MAX_GRID)
#define SDM_TL_LIST 16               // entries of a list of sdm_apply_matte_tiles: SDM_TILES_MAX
#define SDM_TL_BH 16                 // a block of tiles_blend_kernel: 16 rows of 64 pixels, wave v of 4 takes the rows v, v + 4, v + 8, v + 12 (64 rows per block
                                     // were measured slower: a thread's rows are served one after the other, profiles/NOTES.md)
#define SDM_TL_BW 64

struct TilesAxis { int n, d, size; };

// the grid rule of one axis (integers only, truncating division)
static inline TilesAxis tiles_axis(int L, int T, int O) {
  TilesAxis a;
  if (L <= T) { a.n = 1; a.d = 0; a.size = L; }
  else { a.n = (L - O + (T - O) - 1) / (T - O); a.d = L - T; a.size = T; }
  return a;
}
SDM_HD_INLINE int tiles_origin(TilesAxis a, int i) { return a.n > 1 ? (int)(((long long)i * a.d) / (a.n - 1)) : 0; }

// x |= v on a word that other threads OR into at the same time (LDS or global)
#ifdef SDM_EMU
static inline void tiles_or(unsigned int* p, unsigned int v) { std::lock_guard<std::mutex> g(emu::g_atomic_mu); *p |= v; }
#else
SDM_DEV_INLINE void tiles_or(unsigned int* p, unsigned int v) { atomicOr(p, v); }
#endif

__global__ void tiles_init_kernel(unsigned int* __restrict__ flags, int B) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < B * SDM_TL_WORDS) flags[i] = 0u;
}

// the smallest index whose tile ends behind c, and the largest whose tile starts at or in front of c: o[] increases, o[0] = 0 <= c < o[n-1] + size
SDM_DEV_INLINE int tiles_first(const int* o, int n, int size, int c) {
  int a = 0, e = n - 1;
  while (a < e) { const int m = (a + e) >> 1; if (o[m] + size > c) e = m; else a = m + 1; }
  return a;
}
SDM_DEV_INLINE int tiles_last(const int* o, int n, int c) {
  int a = 0, e = n - 1;
  while (a < e) { const int m = (a + e + 1) >> 1; if (o[m] <= c) a = m; else e = m - 1; }
  return a;
}

// The band pixels of row y between the columns xa <= xb (both in the band) mark their cells in the block's bitmask.  For xb - xa < 4 the cells of the
// pixels in between are among those of xa and xb: a tile that holds neither would lie inside (xa, xb), and a tile of a grid with several is >= 16 wide.
// A bit that is set already is not ORed again (a plain read: seeing a stale 0 only repeats the OR).
SDM_DEV_INLINE void tiles_mark_span(const int* oy, const int* ox, TilesAxis ay, TilesAxis ax, int y, int xa, int xb, unsigned int* bits) {
  const int y_lo = tiles_first(oy, ay.n, ay.size, y), y_hi = tiles_last(oy, ay.n, y);
  const int x_lo = tiles_first(ox, ax.n, ax.size, xa), x_hi = tiles_last(ox, ax.n, xb);
  for (int cy = y_lo; cy <= y_hi; ++cy)
    for (int cx = x_lo; cx <= x_hi; ++cx) {
      const int cell = cy * ax.n + cx;
      const unsigned int m = 1u << (cell & 31);
      if (!(((volatile unsigned int*)bits)[cell >> 5] & m)) tiles_or(&bits[cell >> 5], m);
    }
}

// grid: B * ceil(H*W / SDM_ROI_PX) blocks of 256 threads.  VEC: 16-byte loads - W % 4 == 0 (a vector never crosses a row) and the plane 16-byte aligned.
// A pixel is in the band iff lo < v and v < hi (NaN is not); a pixel beyond the image reads as -1, below every lo >= 0.
template <bool VEC>
__global__ __launch_bounds__(256) void tiles_mark_kernel(const float* __restrict__ plane, unsigned int* __restrict__ flags, int B, int H, int W, float lo,
                                                         float hi, TilesAxis ay, TilesAxis ax) {
  SDM_SHARED int oy[SDM_TL_AXIS];
  SDM_SHARED int ox[SDM_TL_AXIS];
  SDM_SHARED unsigned int bits[SDM_TL_WORDS];
  const int tid = threadIdx.x;
  const int HW = H * W, chunks = (HW + SDM_ROI_PX - 1) / SDM_ROI_PX;
  const int b = blockIdx.x / chunks, base = (blockIdx.x - b * chunks) * SDM_ROI_PX;
  const float* pl = plane + (size_t)b * HW;
  for (int i = tid; i < ay.n; i += 256) oy[i] = tiles_origin(ay, i);
  for (int i = tid; i < ax.n; i += 256) ox[i] = tiles_origin(ax, i);
  if (tid < SDM_TL_WORDS) bits[tid] = 0u;
  __syncthreads();
  if (VEC) {
    for (int it = 0; it < 16; it += 4) {
      f32x4 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {      // four loads in flight per thread
        const int i = base + (it + u) * 1024 + tid * 4;
        const f32x4 none = {-1.0f, -1.0f, -1.0f, -1.0f};
        v[u] = i < HW ? *(const f32x4*)(pl + i) : none;
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const bool m0 = lo < v[u][0] && v[u][0] < hi, m1 = lo < v[u][1] && v[u][1] < hi, m2 = lo < v[u][2] && v[u][2] < hi, m3 = lo < v[u][3] && v[u][3] < hi;
        const bool any = m0 || m1 || m2 || m3;
        if (!__any(any)) continue;      // wave-uniform: a wave over definite pixels has nothing to look up
        if (any) {
          const int i = base + (it + u) * 1024 + tid * 4;
          const int y = i / W, x = i - y * W;
          tiles_mark_span(oy, ox, ay, ax, y, x + (m0 ? 0 : m1 ? 1 : m2 ? 2 : 3), x + (m3 ? 3 : m2 ? 2 : m1 ? 1 : 0), bits);
        }
      }
    }
  } else {
    for (int it = 0; it < 64; ++it) {
      const int i = base + it * 256 + tid;
      const float v = i < HW ? pl[i] : -1.0f;
      const bool m = lo < v && v < hi;
      if (!__any(m)) continue;
      if (m) {
        const int y = i / W, x = i - y * W;
        tiles_mark_span(oy, ox, ay, ax, y, x, x, bits);
      }
    }
  }
  __syncthreads();
  if (tid < SDM_TL_WORDS && bits[tid] != 0u) tiles_or(flags + b * SDM_TL_WORDS + tid, bits[tid]);
}

// One thread per image: tiles int32 [B][K][5] = {b, y0, x0, h, w}: the set cells in row-major order, the first K of them; {-1, 0, 0, 0, 0} in every
// further entry.  count (may be NULL) int32 [B]: the number of set cells, also beyond K.
__global__ void tiles_list_kernel(const unsigned int* __restrict__ flags, int* __restrict__ tiles, int* __restrict__ count, int B, int K, TilesAxis ay,
                                  TilesAxis ax) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const unsigned int* f = flags + b * SDM_TL_WORDS;
  int* out = tiles + (size_t)b * K * 5;
  int n = 0;
  for (int cy = 0; cy < ay.n; ++cy)
    for (int cx = 0; cx < ax.n; ++cx) {
      const int cell = cy * ax.n + cx;
      if (!((f[cell >> 5] >> (cell & 31)) & 1u)) continue;
      if (n < K) {
        int* q = out + n * 5;
        q[0] = b; q[1] = tiles_origin(ay, cy); q[2] = tiles_origin(ax, cx); q[3] = ay.size; q[4] = ax.size;
      }
      ++n;
    }
  for (int i = n < K ? n : K; i < K; ++i) {
    out[i * 5] = -1;
    for (int c = 1; c < 5; ++c) out[i * 5 + c] = 0;
  }
  if (count) count[b] = n;
}

// ---- sdm_apply_matte_tiles ---------------------------------------------------------------------------------------------------------------------
// the weight of one axis: o = offset inside the tile of extent `ext` at `start` of a frame axis of length L.  A side on the frame's border does not ramp;
// the others give min(1, (d + 1) / (feather + 1)) with d the distance to that side's edge pixel - the smaller d decides (the division is monotonic),
// and d >= feather is the 1.  fp1 = (float)(feather + 1).
SDM_DEV_INLINE float tiles_axis_weight(int o, int start, int ext, int L, int feather, float fp1) {
  int d = 0x7FFFFFFF;
  if (start != 0) d = o;
  if (start + ext != L) d = min(d, ext - 1 - o);
  return d >= feather ? 1.0f : (float)(d + 1) / fp1;
}

// roi_paste_kernel's value of slot n at the offset (oy, ox) of its h x w tile
SDM_DEV_INLINE float tiles_value(const float* __restrict__ in, int n, int S, int h, int w, int oy, int ox) {
  const float* pl = in + (size_t)n * S * S;
  float x;
  if (h == S && w == S) x = pl[(size_t)oy * S + ox];
  else x = resize_aa_sample([&](int y, int xx) { return pl[(size_t)y * S + xx]; }, S, S, h, w, oy, ox);
  return fminf(fmaxf(x, 0.0f), 1.0f);
}

// The model's alphas [N,S,S] into the frames [B,H,W], each pixel written once.  grid: B * ceil(H / SDM_TL_BH) * ceil(W / SDM_TL_BW) blocks of 256
// threads; a wave stores rows of 64 consecutive pixels.  The sanitised list sits in LDS (boxes_paste_kernel); thread 0 culls it against the block's
// rectangle into `hit` (list order kept), so the pixel loops run over the tiles that can contain the pixel, not over N.  Per pixel, over the tiles that
// do, in list order: Wsum = sum w_i, out = clamp(sum (w_i / Wsum) * a_i, 0, 1), w_i = wy * wx; a pixel in no tile gets the base: base[p] (NaN -> 0,
// clamped) or, without a base plane, 1.0 if trimap[p] > 0.5, else 0.0.
__global__ __launch_bounds__(256) void tiles_blend_kernel(const float* __restrict__ in, const int* __restrict__ list, const float* __restrict__ tri,
                                                          const float* __restrict__ basep, float* __restrict__ out, int N, int B, int H, int W, int S,
                                                          int feather) {
  SDM_SHARED int q[SDM_TL_LIST * 5];
  SDM_SHARED int hit[SDM_TL_LIST];
  SDM_SHARED int nhit;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int bw = (W + SDM_TL_BW - 1) / SDM_TL_BW, bh = (H + SDM_TL_BH - 1) / SDM_TL_BH;
  const int b = blockIdx.x / (bw * bh), r = blockIdx.x - b * (bw * bh);
  const int ya = (r / bw) * SDM_TL_BH, xa = (r % bw) * SDM_TL_BW;
  if (tid < N * 5) q[tid] = list[tid];
  __syncthreads();
  if (tid == 0) {
    int m = 0;
    for (int n = 0; n < N; ++n) {
      const int* e = q + n * 5;      // (a void entry's -1 is no image)
      if (e[0] == b && e[1] < ya + SDM_TL_BH && e[1] + e[3] > ya && e[2] < xa + SDM_TL_BW && e[2] + e[4] > xa) hit[m++] = n;
    }
    nhit = m;
  }
  __syncthreads();
  const int nh = nhit, fx = xa + lane;
  const float fp1 = (float)(feather + 1);
  if (b >= B || fx >= W) return;
  for (int k = 0; k < SDM_TL_BH / 4; ++k) {
    const int fy = ya + wv + 4 * k;
    if (fy >= H) break;
    const size_t i = ((size_t)b * H + fy) * W + fx;
    float wsum = 0.0f;
    int cnt = 0, last = 0;
    for (int j = 0; j < nh; ++j) {
      const int* e = q + hit[j] * 5;
      const int oy = fy - e[1], ox = fx - e[2];
      if (oy < 0 || oy >= e[3] || ox < 0 || ox >= e[4]) continue;
      wsum += tiles_axis_weight(oy, e[1], e[3], H, feather, fp1) * tiles_axis_weight(ox, e[2], e[4], W, feather, fp1);
      ++cnt; last = j;
    }
    float x;
    if (cnt == 0) {
      if (basep) { const float v = basep[i]; x = v != v ? 0.0f : fminf(fmaxf(v, 0.0f), 1.0f); }
      else x = tri[i] > 0.5f ? 1.0f : 0.0f;
    } else {
      // a single tile (most pixels): its share is w / w == 1, so neither the weight nor the quotient is computed, and the loop is its one entry
      const bool one = cnt == 1;
      float acc = 0.0f;
      for (int j = one ? last : 0; j < (one ? last + 1 : nh); ++j) {
        const int n = hit[j];
        const int* e = q + n * 5;
        const int oy = fy - e[1], ox = fx - e[2];
        if (oy < 0 || oy >= e[3] || ox < 0 || ox >= e[4]) continue;
        float share = 1.0f;
        if (!one) share = tiles_axis_weight(oy, e[1], e[3], H, feather, fp1) * tiles_axis_weight(ox, e[2], e[4], W, feather, fp1) / wsum;
        acc += share * tiles_value(in, n, S, e[3], e[4], oy, ox);
      }
      x = fminf(fmaxf(acc, 0.0f), 1.0f);
    }
    out[i] = x;
  }
}
