// k_trimap.h - trimap from a mask on the GPU (sdm_make_trimap / sdm_apply_matte_mask; DESIGN.md 4, "trimap from a mask").
//
//   F = { p : mask[p] > threshold }                                  (one fp32 compare: NaN is background)
//   trimap[p] = 1.0  if p in F  and no pixel of the image outside F lies within distance erode_px of p
//   trimap[p] = 0.0  if p not in F and no pixel of F lies within distance dilate_px of p
//   trimap[p] = 0.5  otherwise
// i.e. erosion / dilation of F by the closed Euclidean disk (dx^2 + dy^2 <= r^2).  Pixels beyond the image border do not exist: they are
// neither foreground nor background.  Integer arithmetic and compares only, so GPU, emulator and the CPU restatement
// (sdmatte_nodes.trimap_from_mask) agree bit for bit.
//
// Two launches, separable in the sense of a distance transform's first phase:
//   trimap_cols_kernel  per pixel, the vertical run distance to the nearest pixel of the OTHER class in its column, saturated at
//                       cap = max(erode_px, dilate_px) + 1, as ONE signed 16-bit plane: +d for pixels of F, -d for the others (a pixel's
//                       distance to its own class is 0, so the sign carries the class and |v| the one distance that is not trivial);
//   trimap_rows_kernel  a pixel of class c with radius r is "unknown" iff some column x + dx, |dx| <= r, holds a pixel of the other class within
//                       vertical distance hmax[|dx|] = floor(sqrt(r^2 - dx^2)) of its row: column x + dx in row y is either of the other class
//                       itself (distance 0) or of class c, and then |v| is that distance.
#pragma once
#include "sdm_common.h"

#define SDM_TRIMAP_COLS_W 64        // columns of a trimap_cols_kernel block: one wave reads / writes 64 consecutive x
#define SDM_TRIMAP_ROWS_W 256       // pixels of a trimap_rows_kernel block: one row segment, one pixel per thread
#define SDM_TRIMAP_RMAX 255         // = SDM_TRIMAP_MAX_RADIUS (include/sdmatte.h)
#define SDM_TRIMAP_NONE 0x7FFF      // "no such pixel" in the row kernel's LDS words: farther than any hmax

// dynamic LDS of trimap_cols_kernel: class bytes of (rows + 2R) x 64 pixels, then the downward distances of rows x 64 pixels (int16)
SDM_HD_INLINE size_t trimap_cols_smem(int rows, int R) { return (size_t)(rows + 2 * R) * SDM_TRIMAP_COLS_W + (size_t)rows * SDM_TRIMAP_COLS_W * 2; }

// grid: B * ceil(H / rows) * ceil(W / 64) blocks of 256 threads; rows % 4 == 0.  Block = 64 columns x `rows` rows; wave w owns rows / 4 of them and
// walks its own R-row halo above and below (from LDS), so waves never wait for one another after the load.
__global__ __launch_bounds__(256) void trimap_cols_kernel(const float* __restrict__ mask, short* __restrict__ plane, int B, int H, int W, float threshold,
                                                          int R, int rows) {
  SDM_DYN_SMEM(smem);
  unsigned char* cls = smem;                                                             // [rows + 2R][64]: 1 in F, 0 not in F, 2 no such pixel
  short* down = (short*)(smem + (size_t)(rows + 2 * R) * SDM_TRIMAP_COLS_W);              // [rows][64] (offset is a multiple of 64 bytes)
  const int tid = threadIdx.x;
  const int nbx = (W + SDM_TRIMAP_COLS_W - 1) / SDM_TRIMAP_COLS_W, nby = (H + rows - 1) / rows;
  const int blk = blockIdx.x;
  const int b = blk / (nbx * nby), by = (blk / nbx) % nby, bx = blk % nbx;
  if (b >= B) return;
  const int x0 = bx * SDM_TRIMAP_COLS_W, y0 = by * rows;
  const float* m = mask + (size_t)b * H * W;
  const int nload = (rows + 2 * R) * SDM_TRIMAP_COLS_W;
  for (int i = tid; i < nload; i += 256) {
    const int y = y0 - R + (i >> 6), x = x0 + (i & 63);
    unsigned char c = 2;
    if (y >= 0 && y < H && x < W) c = (m[(size_t)y * W + x] > threshold) ? 1 : 0;
    cls[i] = c;
  }
  __syncthreads();
  const int col = tid & 63, seg = rows >> 2, cap = R + 1;
  const int r0 = R + (tid >> 6) * seg, r1 = r0 + seg;      // this wave's rows, as row indices of cls
  // upwards from the bottom of the lower halo: dF / dN = distance from the row above the current one down to the nearest pixel of F / not of F
  int dF = cap, dN = cap;
  for (int i = r1 + R - 1; i >= r0; --i) {
    const int c = cls[i * SDM_TRIMAP_COLS_W + col];
    if (i < r1) down[(i - R) * SDM_TRIMAP_COLS_W + col] = (short)(c == 1 ? dN : dF);
    dF = (c == 1) ? 1 : min(dF + 1, cap);
    dN = (c == 0) ? 1 : min(dN + 1, cap);
  }
  // downwards from the top of the upper halo; the smaller of the two distances goes out
  dF = cap; dN = cap;
  const int x = x0 + col;
  for (int i = r0 - R; i < r1; ++i) {
    const int c = cls[i * SDM_TRIMAP_COLS_W + col];
    if (i >= r0) {
      const int y = y0 + i - R;
      const int d = min(c == 1 ? dN : dF, (int)down[(i - R) * SDM_TRIMAP_COLS_W + col]);
      if (y < H && x < W) plane[((size_t)b * H + y) * W + x] = (short)(c == 1 ? d : -d);
    }
    dF = (c == 1) ? 1 : min(dF + 1, cap);
    dN = (c == 0) ? 1 : min(dN + 1, cap);
  }
}

// largest h >= 0 with h^2 <= n (n >= 0, below 2^17): the float root is only a first guess, the two loops make it exact
SDM_DEV_INLINE int trimap_isqrt(int n) {
  int h = (int)sqrtf((float)n);
  while (h * h > n) --h;
  while ((h + 1) * (h + 1) <= n) ++h;
  return h;
}

// grid: B * H * ceil(W / 256) blocks of 256 threads, one pixel per thread.  LDS: the row segment plus R pixels on either side as words
// [distance to the nearest pixel outside F | distance to the nearest pixel of F << 16] (0 for a pixel of that class itself, SDM_TRIMAP_NONE for both
// beyond the image), and the table [hmax_erode[dx] + 1 | (hmax_dilate[dx] + 1) << 16] (0 = dx beyond that radius): "hit" is distance < table entry.
// A wave whose whole window (its 64 pixels + R on either side) lies deeper than the radius inside one class writes that class without scanning;
// every other wave scans dx outwards and stops once each of its pixels is decided.  Both shortcuts skip compares whose outcome is known.
__global__ __launch_bounds__(256) void trimap_rows_kernel(const short* __restrict__ plane, float* __restrict__ trimap, int B, int H, int W, int erode_px,
                                                          int dilate_px) {
  SDM_SHARED unsigned int row[SDM_TRIMAP_ROWS_W + 2 * SDM_TRIMAP_RMAX];
  SDM_SHARED unsigned int tab[SDM_TRIMAP_RMAX + 1];
  const int tid = threadIdx.x;
  const int R = max(erode_px, dilate_px);
  const int nbx = (W + SDM_TRIMAP_ROWS_W - 1) / SDM_TRIMAP_ROWS_W;
  const long blk = blockIdx.x;
  const int bx = (int)(blk % nbx);
  const long line = blk / nbx;                                     // = b * H + y
  if (line >= (long)B * H) return;
  const int xb = bx * SDM_TRIMAP_ROWS_W;
  const short* src = plane + (size_t)line * W;
  for (int i = tid; i < SDM_TRIMAP_ROWS_W + 2 * R; i += 256) {
    const int x = xb - R + i;
    unsigned int w = (unsigned int)SDM_TRIMAP_NONE | ((unsigned int)SDM_TRIMAP_NONE << 16);
    if (x >= 0 && x < W) {
      const int v = src[x];
      w = (unsigned int)max(v, 0) | ((unsigned int)max(-v, 0) << 16);
    }
    row[i] = w;
  }
  if (tid <= R) {
    const unsigned int he = tid <= erode_px ? (unsigned int)trimap_isqrt(erode_px * erode_px - tid * tid) + 1u : 0u;
    const unsigned int hd = tid <= dilate_px ? (unsigned int)trimap_isqrt(dilate_px * dilate_px - tid * tid) + 1u : 0u;
    tab[tid] = he | (hd << 16);
  }
  __syncthreads();
  const int x = xb + tid;
  const bool valid = x < W;
  const unsigned int own = row[R + tid];
  const bool fg = (own & 0xFFFFu) != 0u;                           // a pixel of F is at distance >= 1 from the pixels outside F
  // wave window: entries [w0, w0 + 64 + 2R) of row[]
  const int lane = tid & 63, w0 = tid & ~63;
  int shallow_f = 0, shallow_n = 0;                                // some entry within erode_px of a pixel outside F / within dilate_px of a pixel of F
  for (int i = lane; i < 64 + 2 * R; i += 64) {
    const unsigned int w = row[w0 + i];
    shallow_f |= (int)((w & 0xFFFFu) <= (unsigned int)erode_px);
    shallow_n |= (int)((w >> 16) <= (unsigned int)dilate_px);
  }
  shallow_f = __any(shallow_f);
  shallow_n = __any(shallow_n);
  if (!shallow_f) { if (valid) trimap[(size_t)line * W + x] = 1.0f; return; }      // every pixel of the window is of F, deeper than erode_px
  if (!shallow_n) { if (valid) trimap[(size_t)line * W + x] = 0.0f; return; }
  const int sh = fg ? 0 : 16, r = fg ? erode_px : dilate_px;
  bool hit = ((own >> sh) & 0xFFFFu) < ((tab[0] >> sh) & 0xFFFFu);
  for (int dx = 1; dx <= R; ++dx) {
    if (!__any((int)(valid && !hit && dx <= r))) break;
    const unsigned int t = (tab[dx] >> sh) & 0xFFFFu;
    const unsigned int a = (row[R + tid - dx] >> sh) & 0xFFFFu, c = (row[R + tid + dx] >> sh) & 0xFFFFu;
    hit = hit || a < t || c < t;
  }
  if (valid) trimap[(size_t)line * W + x] = hit ? 0.5f : (fg ? 1.0f : 0.0f);
}
