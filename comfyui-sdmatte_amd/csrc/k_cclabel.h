// k_cclabel.h - connected-component labelling for sdm_clean_mask (include/sdmatte.h; DESIGN.md 4, "clean masks").
//
// A class plane (stage A: mask > threshold, 8-connected; stage B: NOT (out > threshold), 4-connected) is labelled with a union-find over global
// memory.  A label is the GLOBAL pixel index (b*H*W + y*W + x) of a pixel of the same component, never larger than the pixel's own index, and -1
// outside the class; a root is a pixel whose label is its own index.  Every union makes the smaller root the parent, so the root of a finished
// component is its smallest pixel index.  Launches per labelling, whatever B, H, W and the content:
//   cc_tile_kernel     one block per 64 x 64 tile: labels the tile in LDS, writes the global index of every pixel's tile-local root, zeroes the area words
//   cc_seam_kernel     one block per tile: unions across the tile's top, left and right seam (atomicMin on the label plane)
//   cc_flatten_kernel  root[p] = find(p) into a SECOND plane (the label plane is only read), area[root] += pixels, combined per run of a wave and then
//                      per block first; stage B: a component that touches the image border gets area >= SDM_CC_BORDER
// then cc_select_kernel (twice: largest area per image, smallest root of that area), cc_apply_kernel and cc_fill_kernel use root / area.
// No block waits for another one: the only loops are chains of labels, and labels only decrease.
// Planes: label int32, root int32, area int32 (indexed by the root's pixel index) = 12 bytes per pixel of the batch.
//
// Which neighbours a pixel p unions with (the others follow by transitivity; W, N, NW, NE = "that neighbour exists and is of the class"):
//   W  always (inside a tile: the row runs of the tile kernel);
//   N  unless W and NW (then W ~ NW is W's own N union, and NW ~ N lie side by side);
//   without N, 8-connected only: NW unless W (W's N is NW), and NE.
// The tile kernel applies the rule to the neighbours inside the tile (a pixel beyond the tile counts as absent, which only adds unions), the seam
// kernel to the neighbours in other tiles.
#pragma once
#include "sdm_common.h"

#define SDM_CC_T 64                 // tile side
#define SDM_CC_PX 1024              // pixels of a block of the flat kernels: 256 threads x 4 consecutive pixels
#define SDM_CC_BORDER 0x40000000u   // area word of a component that touches the image border (areas proper are <= 2^28 = SDM_FG_MAX_PIXELS)

// root of r.  The loads are volatile: other blocks lower labels while this one reads.  A stale value is an earlier label of the same word, i.e. a
// pixel of the same component with a larger index than the current label, so the walk is still strictly downwards inside the component.
SDM_DEV_INLINE int cc_find(const volatile int* label, int r) {
  int l;
  while ((l = label[r]) != r) r = l;      // ends: l < r at every step
  return r;
}

// Joins the components of a and b.  Labels only ever decrease (atomicMin) and are >= 0, so every loop here ends: a retry means that label[a] was
// already below a, i.e. another union lowered it since this thread read it, and there are finitely many such steps.
SDM_DEV_INLINE void cc_union(int* label, int a, int b) {
  for (;;) {
    a = cc_find(label, a);
    b = cc_find(label, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }      // a > b: a hangs itself below b
    const int old = atomicMin(&label[a], b);
    if (old == a) return;                              // a was a root and now points to b
    // a was no root any more (old < a).  If b < old the word now holds b and the link a -> old is gone: union(old, b) restores it; otherwise a still
    // points to old, and union(old, b) is what remains to do.  Either way:
    a = old;
  }
}

// grid: B * ceil(H / 64) * ceil(W / 64) blocks of 256 threads.  cls(p) = (src[p] > threshold) != invert; pixels beyond the image are outside the class.
// sel / stats (stage A only, may be NULL): the first tile of every image resets that image's selection words {largest area, its smallest root} and
// the four statistics; later launches only add to them.
__global__ __launch_bounds__(256) void cc_tile_kernel(const float* __restrict__ src, int* __restrict__ label, int* __restrict__ area, int B, int H, int W,
                                                      float threshold, int invert, int conn8, int* __restrict__ sel, int* __restrict__ stats) {
  SDM_SHARED int lab[SDM_CC_T * SDM_CC_T];      // label = index inside the tile (ly * 64 + lx), -1 outside the class
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int nbx = (W + SDM_CC_T - 1) / SDM_CC_T, nby = (H + SDM_CC_T - 1) / SDM_CC_T;
  const int blk = blockIdx.x;
  const int b = blk / (nbx * nby), by = (blk / nbx) % nby, bx = blk % nbx;
  if (b >= B) return;
  const int x0 = bx * SDM_CC_T, y0 = by * SDM_CC_T;
  const int base = b * H * W;
  if (by == 0 && bx == 0) {
    if (sel && tid == 0) { sel[2 * b] = 0; sel[2 * b + 1] = 0x7FFFFFFF; }
    if (stats && tid < 4) stats[4 * b + tid] = 0;
  }
  // rows: wave w owns rows 16w .. 16w + 15, one pixel per lane; a pixel's first label is the start of its row run (prefix maximum of the run heads)
  const int x = x0 + lane;
  for (int k = 0; k < 16; ++k) {
    const int ly = wv * 16 + k, y = y0 + ly;
    if (y >= H) { lab[ly * SDM_CC_T + lane] = -1; continue; }      // (the same for the whole wave)
    int c = 0;
    if (x < W) {
      const int g = base + y * W + x;
      c = ((src[g] > threshold) ? 1 : 0) ^ invert;
      area[g] = 0;
    }
    const int cprev = __shfl(c, max(lane - 1, 0));
    int s = (c && (lane == 0 || !cprev)) ? lane : -1;
    for (int d = 1; d < 64; d <<= 1) {
      const int o = __shfl(s, max(lane - d, 0));
      if (lane >= d) s = max(s, o);
    }
    lab[ly * SDM_CC_T + lane] = c ? ly * SDM_CC_T + s : -1;
  }
  __syncthreads();
  // unions with the row above.  (lab[i] >= 0 is the class of i at any time: unions never change a sign.)
  for (int i = tid; i < SDM_CC_T * SDM_CC_T; i += 256) {
    const int lx = i & 63;
    if (i < SDM_CC_T || ((volatile int*)lab)[i] < 0) continue;
    const volatile int* vl = lab;
    const bool n = vl[i - 64] >= 0, w = lx > 0 && vl[i - 1] >= 0, nw = lx > 0 && vl[i - 65] >= 0;
    if (n) {
      if (!(w && nw)) cc_union(lab, i, i - 64);
    } else if (conn8) {
      if (nw && !w) cc_union(lab, i, i - 65);
      if (lx < 63 && vl[i - 63] >= 0) cc_union(lab, i, i - 63);
    }
  }
  __syncthreads();
  for (int i = tid; i < SDM_CC_T * SDM_CC_T; i += 256) {
    const int y = y0 + (i >> 6), xx = x0 + (i & 63);
    if (y >= H || xx >= W) continue;
    int out = -1;
    if (lab[i] >= 0) {
      const int r = cc_find(lab, i);
      out = base + (y0 + (r >> 6)) * W + x0 + (r & 63);
    }
    label[base + y * W + xx] = out;
  }
}

// grid: one block of 256 threads per tile; threads 0..63 the tile's top row, 64..127 its left column, 128..191 its right column (rows 1..63 of both).
__global__ __launch_bounds__(256) void cc_seam_kernel(int* __restrict__ label, int B, int H, int W, int conn8) {
  const int tid = threadIdx.x, side = tid >> 6, k = tid & 63;
  const int nbx = (W + SDM_CC_T - 1) / SDM_CC_T, nby = (H + SDM_CC_T - 1) / SDM_CC_T;
  const int blk = blockIdx.x;
  const int b = blk / (nbx * nby), by = (blk / nbx) % nby, bx = blk % nbx;
  if (b >= B || side > 2 || (side > 0 && k == 0) || (side == 2 && !conn8)) return;
  const int ly = side == 0 ? 0 : k, lx = side == 0 ? k : (side == 1 ? 0 : 63);
  const int y = by * SDM_CC_T + ly, x = bx * SDM_CC_T + lx;
  if (y >= H || x >= W) return;
  const int p = b * H * W + y * W + x;
  const volatile int* vl = label;
  if (vl[p] < 0) return;
  const bool oN = ly == 0, oW = lx == 0;                       // that neighbour lies in another tile
  const bool w = x > 0 && vl[p - 1] >= 0, n = y > 0 && vl[p - W] >= 0, nw = x > 0 && y > 0 && vl[p - W - 1] >= 0;
  // W across the seam, unless N (inside this tile, so p ~ N is the tile kernel's) and NW: N ~ NW is then N's own W union, one row up
  if (w && oW && !(n && nw && !oN)) cc_union(label, p, p - 1);
  if (n) {
    if (oN && !(w && nw)) cc_union(label, p, p - W);
  } else if (conn8) {
    if (nw && !w && (oN || oW)) cc_union(label, p, p - W - 1);
    if ((oN || lx == 63) && y > 0 && x + 1 < W && vl[p - W + 1] >= 0) cc_union(label, p, p - W + 1);
  }
}

// sum of v over the run of consecutive lanes that hold the same key, returned in the run's first lane (`head`); the other lanes get partial sums
SDM_DEV_INLINE int cc_run_sum(int key, int v, bool& head) {
  const int lane = threadIdx.x & 63;
  const int kprev = __shfl(key, max(lane - 1, 0)), knext = __shfl(key, min(lane + 1, 63));
  head = lane == 0 || kprev != key;
  int stop = (lane == 63 || knext != key) ? 1 : 0;              // the lanes summed so far reach the end of the run
  for (int d = 1; d < 64; d <<= 1) {
    const int ov = __shfl(v, min(lane + d, 63)), os = __shfl(stop, min(lane + d, 63));
    if (!stop) { v += ov; stop = os; }                          // (not stopped: lane + d is inside the run, so inside the wave)
  }
  return v;
}

SDM_DEV_INLINE int cc_wave_sum(int v) {
  for (int d = 1; d < 64; d <<= 1) v += __shfl_xor(v, d);
  return v;
}

// the 4 consecutive pixels pl0 .. pl0 + 3 of image b as a 16-byte load where the whole run exists and `vec` (H*W % 4 == 0, aligned plane)
SDM_DEV_INLINE void cc_load4(const int* __restrict__ plane, int base, int pl0, int HW, int vec, int (&v)[4]) {
  if (vec && pl0 + 3 < HW) {
    const i32x4 q = *(const i32x4*)(plane + base + pl0);
    v[0] = q[0]; v[1] = q[1]; v[2] = q[2]; v[3] = q[3];
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = pl0 + j < HW ? plane[base + pl0 + j] : -1;
  }
}

// One pixel count (or border mark) for root r: into the block's table if r owns or can claim its slot, straight to memory otherwise.
SDM_DEV_INLINE void cc_area_add(int* hkey, int* hcnt, int* __restrict__ area, int r, int v) {
  const int slot = (int)(((unsigned int)r * 2654435761u) >> 26);      // 64 slots
  const unsigned int old = atomicCAS((unsigned int*)&hkey[slot], 0xFFFFFFFFu, (unsigned int)r);
  if (old == 0xFFFFFFFFu || old == (unsigned int)r) {
    if (v >> 16) atomicMax((unsigned int*)&hcnt[slot], SDM_CC_BORDER);      // (>= SDM_CC_BORDER from here on, whatever is added: at most 2^28 more)
    else atomicAdd(&hcnt[slot], v);
  } else if (v >> 16) atomicMax((unsigned int*)&area[r], SDM_CC_BORDER);
  else atomicAdd(&area[r], v);
}

// grid: B * ceil(H*W / SDM_CC_FLAT_PX) blocks of 256 threads (no block spans two images); a block walks its 8 chunks of 1024 pixels in turn.  label is
// read with plain loads only: nothing writes it in this launch.  border != 0 (stage B): a pixel of the class on the image border marks its component.
// stats (stage A, may be NULL): [b][0] += roots of image b.
// Areas are combined three times before they reach memory, so that a component of millions of pixels is not millions of atomics on one word: the 4 pixels
// of a thread, the run of lanes with the same root (256 pixels inside a large component), then a 64-slot table of the block in LDS, keyed by the root
// and flushed once at the end - a root that finds its slot taken by another one goes to memory directly.
#define SDM_CC_FLAT_CHUNKS 8
#define SDM_CC_FLAT_PX (SDM_CC_FLAT_CHUNKS * SDM_CC_PX)
__global__ __launch_bounds__(256) void cc_flatten_kernel(const int* __restrict__ label, int* __restrict__ root, int* __restrict__ area, int B, int H, int W,
                                                         int border, int vec, int* __restrict__ stats) {
  SDM_SHARED int hkey[64];
  SDM_SHARED int hcnt[64];
  const int HW = H * W, nblk = (HW + SDM_CC_FLAT_PX - 1) / SDM_CC_FLAT_PX;
  const int b = blockIdx.x / nblk, first = (blockIdx.x % nblk) * SDM_CC_FLAT_CHUNKS;
  if (b >= B) return;
  if (threadIdx.x < 64) { hkey[threadIdx.x] = -1; hcnt[threadIdx.x] = 0; }
  __syncthreads();
  const int base = b * HW;
  int nroots = 0;
  for (int chunk = first; chunk < first + SDM_CC_FLAT_CHUNKS; ++chunk) {
    const int pl0 = chunk * SDM_CC_PX + threadIdx.x * 4;      // (may lie beyond the image: such a thread has no pixel, but takes part in the wave's exchanges)
    int l[4], r[4];
    cc_load4(label, base, min(pl0, HW), HW, vec, l);
    int nbord = 0;
    int y = 0, x = 0;
    if (border && pl0 < HW) { y = pl0 / W; x = pl0 - y * W; }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (l[j] < 0) r[j] = -1;
      else if (j > 0 && l[j] == l[j - 1]) r[j] = r[j - 1];
      else { int q = l[j], t; while ((t = label[q]) != q) q = t; r[j] = q; }      // ends: t < q at every step
      if (r[j] == base + pl0 + j) ++nroots;
      if (border) {
        if (r[j] >= 0 && (y == 0 || y == H - 1 || x == 0 || x == W - 1)) nbord |= 1 << j;
        if (++x == W) { x = 0; ++y; }
      }
    }
    if (vec && pl0 + 3 < HW) {
      i32x4 q; q[0] = r[0]; q[1] = r[1]; q[2] = r[2]; q[3] = r[3];
      *(i32x4*)(root + base + pl0) = q;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) if (pl0 + j < HW) root[base + pl0 + j] = r[j];
    }
    // a thread whose 4 pixels share one root hands them to the run of lanes with that root; any other thread adds its pixels one by one
    const bool whole = r[0] >= 0 && r[0] == r[1] && r[0] == r[2] && r[0] == r[3];
    if (!whole) {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (r[j] >= 0) cc_area_add(hkey, hcnt, area, r[j], ((nbord >> j) & 1) ? 0x10000 : 1);
    }
    bool head;
    const int v = cc_run_sum(whole ? r[0] : -1, whole ? (4 | (nbord ? 0x10000 : 0)) : 0, head);
    if (whole && head) cc_area_add(hkey, hcnt, area, r[0], v);
  }
  __syncthreads();
  if (threadIdx.x < 64 && hkey[threadIdx.x] >= 0) {
    const int r = hkey[threadIdx.x], v = hcnt[threadIdx.x];
    if ((unsigned int)v >= SDM_CC_BORDER) atomicMax((unsigned int*)&area[r], SDM_CC_BORDER);
    else atomicAdd(&area[r], v);
  }
  if (stats) {
    nroots = cc_wave_sum(nroots);
    if ((threadIdx.x & 63) == 0 && nroots) atomicAdd(&stats[4 * b], nroots);
  }
}

// grid: B * ceil(H*W / 1024) blocks of 256 threads (no block spans two images).  phase 0: sel[b][0] = largest area among the roots of image b; phase 1: sel[b][1] = smallest root of that area.
__global__ __launch_bounds__(256) void cc_select_kernel(const int* __restrict__ root, const int* __restrict__ area, int B, int H, int W, int phase, int vec,
                                                        int* __restrict__ sel) {
  const int HW = H * W, nchunk = (HW + SDM_CC_PX - 1) / SDM_CC_PX;
  const int b = blockIdx.x / nchunk, chunk = blockIdx.x % nchunk;
  if (b >= B) return;
  const int base = b * HW, pl0 = chunk * SDM_CC_PX + threadIdx.x * 4;
  int r[4];
  cc_load4(root, base, pl0, HW, vec, r);
  const int best = phase ? sel[2 * b] : 0;
  int m = phase ? 0x7FFFFFFF : 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (r[j] != base + pl0 + j) continue;      // roots only (-1 never equals an index)
    const int a = area[r[j]];
    if (!phase) m = max(m, a);
    else if (a == best) m = min(m, r[j]);
  }
  for (int d = 1; d < 64; d <<= 1) { const int o = __shfl_xor(m, d); m = phase ? min(m, o) : max(m, o); }
  if ((threadIdx.x & 63) != 0) return;
  if (!phase) { if (m > 0) atomicMax((unsigned int*)&sel[2 * b], (unsigned int)m); }
  else if (m != 0x7FFFFFFF) atomicMin(&sel[2 * b + 1], m);
}

SDM_DEV_INLINE void cc_add_stats(int* __restrict__ stats, int b, int slot, int ncomp, int npix) {
  ncomp = cc_wave_sum(ncomp);
  npix = cc_wave_sum(npix);
  if ((threadIdx.x & 63) == 0) {
    if (ncomp) atomicAdd(&stats[4 * b + slot], ncomp);
    if (npix) atomicAdd(&stats[4 * b + 3], npix);
  }
}

// Stage A's result, or the plain threshold / copy when stage_a == 0 (root, area, sel unused).  grid as cc_select_kernel.
//   out = 0 for a pixel of a removed component; otherwise mask, or (mask > threshold) as 1.0 / 0.0 when binarize.
// vec: 16-byte runs (H*W % 4 == 0 and mask, out, root aligned).  stats (may be NULL): [b][1] += removed components, [b][3] += removed pixels.
__global__ __launch_bounds__(256) void cc_apply_kernel(const float* __restrict__ mask, const int* __restrict__ root, const int* __restrict__ area,
                                                       const int* __restrict__ sel, float* __restrict__ out, int B, int H, int W, float threshold, int stage_a,
                                                       int min_area, int keep_largest, int binarize, int vec, int* __restrict__ stats) {
  const int HW = H * W, nchunk = (HW + SDM_CC_PX - 1) / SDM_CC_PX;
  const int b = blockIdx.x / nchunk, chunk = blockIdx.x % nchunk;
  if (b >= B) return;
  const int base = b * HW, pl0 = chunk * SDM_CC_PX + threadIdx.x * 4;
  const bool v4 = vec && pl0 + 3 < HW;
  float m[4];
  int r[4] = {-1, -1, -1, -1};
  if (v4) {
    const f32x4 q = *(const f32x4*)(mask + base + pl0);
    m[0] = q[0]; m[1] = q[1]; m[2] = q[2]; m[3] = q[3];
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) m[j] = pl0 + j < HW ? mask[base + pl0 + j] : 0.0f;
  }
  if (stage_a) cc_load4(root, base, pl0, HW, vec, r);
  const int keep_root = (stage_a && keep_largest) ? sel[2 * b + 1] : -1;
  int ncomp = 0, npix = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const bool fg = m[j] > threshold;
    bool removed = false;
    if (stage_a && fg && r[j] >= 0) removed = area[r[j]] < min_area || (keep_largest && r[j] != keep_root);
    if (removed) { ++npix; if (r[j] == base + pl0 + j) ++ncomp; }
    if (removed) m[j] = 0.0f;
    else if (binarize) m[j] = fg ? 1.0f : 0.0f;
  }
  if (v4) {
    f32x4 q; q[0] = m[0]; q[1] = m[1]; q[2] = m[2]; q[3] = m[3];
    *(f32x4*)(out + base + pl0) = q;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) if (pl0 + j < HW) out[base + pl0 + j] = m[j];
  }
  if (stats && stage_a) cc_add_stats(stats, b, 1, ncomp, npix);
}

// Stage B's result: 1.0 into every pixel of a background component that does not touch the border and has area <= max_hole_area; nothing else is
// written (and `out` is not read).  grid as cc_select_kernel.  stats (may be NULL): [b][2] += filled holes, [b][3] += filled pixels.
__global__ __launch_bounds__(256) void cc_fill_kernel(const int* __restrict__ root, const int* __restrict__ area, float* __restrict__ out, int B, int H, int W,
                                                      int max_hole_area, int vec, int* __restrict__ stats) {
  const int HW = H * W, nchunk = (HW + SDM_CC_PX - 1) / SDM_CC_PX;
  const int b = blockIdx.x / nchunk, chunk = blockIdx.x % nchunk;
  if (b >= B) return;
  const int base = b * HW, pl0 = chunk * SDM_CC_PX + threadIdx.x * 4;
  int r[4];
  cc_load4(root, base, pl0, HW, vec, r);
  int ncomp = 0, npix = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (r[j] < 0) continue;
    if ((unsigned int)area[r[j]] > (unsigned int)max_hole_area) continue;      // (a border component's word is >= SDM_CC_BORDER)
    out[base + pl0 + j] = 1.0f;
    ++npix;
    if (r[j] == base + pl0 + j) ++ncomp;
  }
  if (stats) cc_add_stats(stats, b, 2, ncomp, npix);
}
