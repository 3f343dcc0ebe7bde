// k_boxes.h - a box per subject and the node call over a list of boxes (sdm_subject_boxes / sdm_apply_matte_boxes in include/sdmatte.h; DESIGN.md 4,
// "matte every subject on its own").
//
// sdm_subject_boxes: the components of U = { p : plane[p] > roi_threshold } are labelled by k_cclabel.h (tile, seam, flatten: root[p] = smallest
// pixel index of p's component, area[root] = its pixel count), then, with K = max_boxes and a state of SDM_BX_STRIDE ints per image:
//   boxes_init_kernel      the state's neutral elements
//   boxes_rank_kernel      twice per own slot k = 0 .. K-2, over the roots (root[p] == p) that no earlier slot took: phase 0 the largest area >= min_area
//                          (atomicMax), phase 1 the smallest root of that area (atomicMin) - cc_select_kernel with a list of roots to leave out
//   boxes_reduce_kernel    one read of the root plane: the extrema {ymin, xmin, ymax, xmax} of every chosen component at once, roi_reduce_kernel's
//                          pattern with SDM_BX_SLOTS slots - per thread, per wave (a wave skips the shuffles of a slot it did not see), per block (LDS),
//                          then at most four atomics per slot and block, none for a slot the block did not see
//   boxes_own_kernel       one thread per image: box(C_i) in rank order (roi_axis / roi_square_axis of k_roi.h), dropped if C_i's raw extrema lie inside
//                          a kept box
//   boxes_rest_kernel      a second read of the root plane: the extrema of R, the pixels of U in none of the kept boxes
//   boxes_finalize_kernel  one thread per image: the entries {b, y0, x0, h, w}, the void entries and the count
// 3 + 1 + 2 (K - 1) + 4 launches, whatever B, H, W and the content.  32-bit atomicMin(int) / atomicMax(unsigned) only; integer arithmetic only.
//
// sdm_apply_matte_boxes: boxes_sanitize_kernel copies the caller's list into the arena and voids every entry that does not lie inside the planes, so
// that no later kernel reads outside them whatever the list holds; boxes_prep_image_kernel / boxes_prep_trimap_kernel are roi_prep_image_kernel /
// roi_prep_trimap_kernel with the image index read from the entry (a void slot is fed the whole frame of image 0); boxes_paste_kernel writes every frame
// pixel once: the maximum over the valid boxes that contain it of roi_paste_kernel's value, 0.0 without one.
#pragma once
#include "sdm_common.h"
#include "k_cclabel.h"
#include "k_roi.h"

#define SDM_BX_SLOTS 7               // own components per image: SDM_BOXES_MAX - 1
#define SDM_BX_SEL 0                 // state: [slot][2] = {area, root} of the slot's component ({0, SDM_ROI_NONE}: none)
#define SDM_BX_EXT 16                //        [slot][4] = raw extrema of the slot's component; slot SDM_BX_SLOTS: of the rest R
#define SDM_BX_KEPT 48               //        [i][4] = {y0, x0, h, w} of the kept boxes, in rank order
#define SDM_BX_NKEPT 76              //        their number
#define SDM_BX_STRIDE 80
#define SDM_BX_LIST 16               // entries of a list of sdm_apply_matte_boxes: SDM_BOXES_MAX_TOTAL

__global__ void boxes_init_kernel(int* __restrict__ state, int B) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * SDM_BX_STRIDE) return;
  const int k = i % SDM_BX_STRIDE;
  int v = 0;
  if (k < SDM_BX_EXT) v = (k & 1) && k < 2 * SDM_BX_SLOTS ? SDM_ROI_NONE : 0;
  else if (k < SDM_BX_KEPT) v = (k & 3) < 2 ? SDM_ROI_NONE : 0;
  state[i] = v;
}

// grid as cc_select_kernel: B * ceil(H*W / 1024) blocks of 256 threads.  Slot k of every image: phase 0 sel[k][0] = largest area >= min_area among the
// roots that slots 0 .. k-1 did not take, phase 1 sel[k][1] = smallest such root of that area.  No candidate left: the slot stays {0, SDM_ROI_NONE}.
__global__ __launch_bounds__(256) void boxes_rank_kernel(const int* __restrict__ root, const int* __restrict__ area, int B, int H, int W, int k, int phase,
                                                         int min_area, int vec, int* __restrict__ state) {
  const int HW = H * W, nchunk = (HW + SDM_CC_PX - 1) / SDM_CC_PX;
  const int b = blockIdx.x / nchunk, chunk = blockIdx.x % nchunk;
  if (b >= B) return;
  const int base = b * HW, pl0 = chunk * SDM_CC_PX + threadIdx.x * 4;
  int* sel = state + b * SDM_BX_STRIDE + SDM_BX_SEL;
  int r[4], taken[SDM_BX_SLOTS];
  cc_load4(root, base, pl0, HW, vec, r);
#pragma unroll
  for (int q = 0; q < SDM_BX_SLOTS; ++q) taken[q] = q < k ? sel[2 * q + 1] : SDM_ROI_NONE;      // (no root equals SDM_ROI_NONE)
  const int best = phase ? sel[2 * k] : 0;
  int m = phase ? SDM_ROI_NONE : 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (r[j] != base + pl0 + j) continue;      // roots only (-1 never equals an index)
    bool free_ = true;
#pragma unroll
    for (int q = 0; q < SDM_BX_SLOTS; ++q) free_ = free_ && r[j] != taken[q];
    if (!free_) continue;
    const int a = area[r[j]];
    if (!phase) { if (a >= min_area) m = max(m, a); }
    else if (a == best) m = min(m, r[j]);
  }
  for (int d = 1; d < 64; d <<= 1) { const int o = __shfl_xor(m, d); m = phase ? min(m, o) : max(m, o); }
  if ((threadIdx.x & 63) != 0) return;
  if (!phase) { if (m > 0) atomicMax((unsigned int*)&sel[2 * k], (unsigned int)m); }
  else if (m != SDM_ROI_NONE) atomicMin(&sel[2 * k + 1], m);
}

// 16 consecutive-in-time loads of a block of the two reductions: vector u of thread tid in round it (VEC), as roi_reduce_kernel lays them out
SDM_DEV_INLINE i32x4 boxes_load4(const int* __restrict__ pl, int i, int HW) {
  const i32x4 none = {-1, -1, -1, -1};
  return i < HW ? *(const i32x4*)(pl + i) : none;
}

// grid: B * ceil(H*W / SDM_ROI_PX) blocks of 256 threads.  VEC: 16-byte loads - W % 4 == 0 (a vector never crosses a row; the root plane is an arena
// tensor, so aligned).  A pixel beyond the image reads as -1, the root of a pixel outside U.  The maxima are >= 0: unsigned atomicMax.
template <bool VEC>
__global__ __launch_bounds__(256) void boxes_reduce_kernel(const int* __restrict__ root, int* __restrict__ state, int B, int H, int W) {
  SDM_SHARED int red[4 * SDM_BX_SLOTS * 4];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int HW = H * W, chunks = (HW + SDM_ROI_PX - 1) / SDM_ROI_PX;
  const int b = blockIdx.x / chunks, base = (blockIdx.x - b * chunks) * SDM_ROI_PX;
  if (b >= B) return;
  int* st = state + b * SDM_BX_STRIDE;
  const int* pl = root + (size_t)b * HW;
  int sr[SDM_BX_SLOTS], ymin[SDM_BX_SLOTS], xmin[SDM_BX_SLOTS], ymax[SDM_BX_SLOTS], xmax[SDM_BX_SLOTS];
#pragma unroll
  for (int s = 0; s < SDM_BX_SLOTS; ++s) { sr[s] = st[SDM_BX_SEL + 2 * s + 1]; ymin[s] = xmin[s] = SDM_ROI_NONE; ymax[s] = xmax[s] = -1; }
  if (sr[0] == SDM_ROI_NONE) return;      // no own component in this image (the slots fill in order): the same for the whole block
  if (VEC) {
    for (int it = 0; it < 16; it += 4) {
      i32x4 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = boxes_load4(pl, base + (it + u) * 1024 + tid * 4, HW);      // four loads in flight per thread
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (v[u][0] < 0 && v[u][1] < 0 && v[u][2] < 0 && v[u][3] < 0) continue;      // nothing of U
        const int i = base + (it + u) * 1024 + tid * 4;
        const int y = i / W, x = i - y * W;
#pragma unroll
        for (int s = 0; s < SDM_BX_SLOTS; ++s) {
          const bool m0 = v[u][0] == sr[s], m1 = v[u][1] == sr[s], m2 = v[u][2] == sr[s], m3 = v[u][3] == sr[s];
          if (m0 || m1 || m2 || m3) {
            ymin[s] = min(ymin[s], y); ymax[s] = max(ymax[s], y);
            xmin[s] = min(xmin[s], x + (m0 ? 0 : m1 ? 1 : m2 ? 2 : 3));
            xmax[s] = max(xmax[s], x + (m3 ? 3 : m2 ? 2 : m1 ? 1 : 0));
          }
        }
      }
    }
  } else {
    for (int it = 0; it < 64; ++it) {
      const int i = base + it * 256 + tid;
      const int r = i < HW ? pl[i] : -1;
      if (r < 0) continue;
      const int y = i / W, x = i - y * W;
#pragma unroll
      for (int s = 0; s < SDM_BX_SLOTS; ++s)
        if (r == sr[s]) { ymin[s] = min(ymin[s], y); ymax[s] = max(ymax[s], y); xmin[s] = min(xmin[s], x); xmax[s] = max(xmax[s], x); }
    }
  }
#pragma unroll
  for (int s = 0; s < SDM_BX_SLOTS; ++s) {
    if (__any(ymax[s] >= 0)) {      // wave-uniform: a wave that saw nothing of slot s skips its 24 shuffles
#pragma unroll
      for (int d = 32; d > 0; d >>= 1) {
        ymin[s] = min(ymin[s], __shfl_xor(ymin[s], d)); xmin[s] = min(xmin[s], __shfl_xor(xmin[s], d));
        ymax[s] = max(ymax[s], __shfl_xor(ymax[s], d)); xmax[s] = max(xmax[s], __shfl_xor(xmax[s], d));
      }
    }
    if (lane == 0) {
      int* q = red + (wv * SDM_BX_SLOTS + s) * 4;
      q[0] = ymin[s]; q[1] = xmin[s]; q[2] = ymax[s]; q[3] = xmax[s];
    }
  }
  __syncthreads();
  if (tid < SDM_BX_SLOTS * 4) {
    const int s = tid >> 2, c = tid & 3, w4 = SDM_BX_SLOTS * 4;
    const int* q = red + s * 4;
    if (max(max(q[2], q[w4 + 2]), max(q[2 * w4 + 2], q[3 * w4 + 2])) < 0) return;      // no pixel of slot s in this block: no atomic
    int* dst = st + SDM_BX_EXT + s * 4 + c;
    if (c < 2) atomicMin(dst, min(min(q[c], q[w4 + c]), min(q[2 * w4 + c], q[3 * w4 + c])));
    else atomicMax((unsigned int*)dst, (unsigned int)max(max(q[c], q[w4 + c]), max(q[2 * w4 + c], q[3 * w4 + c])));
  }
}

// box(X) of sdm_subject_roi from X's extrema: margins, clipping, the optional square (roi_finalize_kernel's arithmetic)
SDM_DEV_INLINE void boxes_box(const int* __restrict__ raw, int H, int W, int margin_px, int margin_pct, int square, int* box) {
  int y0, x0, h, w;
  roi_axis(raw[0], raw[2], H, margin_px, margin_pct, &y0, &h);
  roi_axis(raw[1], raw[3], W, margin_px, margin_pct, &x0, &w);
  if (square) {
    const int L = max(h, w);
    roi_square_axis(L, H, &y0, &h);
    roi_square_axis(L, W, &x0, &w);
  }
  box[0] = y0; box[1] = x0; box[2] = h; box[3] = w;
}

// One thread per image.  The own components in rank order: C_i gets box(C_i) unless its raw extrema lie inside the box of a kept C_j, j < i.
__global__ void boxes_own_kernel(int* __restrict__ state, int B, int H, int W, int margin_px, int margin_pct, int square) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  int* st = state + b * SDM_BX_STRIDE;
  int nk = 0;
  for (int i = 0; i < SDM_BX_SLOTS; ++i) {
    if (st[SDM_BX_SEL + 2 * i + 1] == SDM_ROI_NONE) break;
    const int* raw = st + SDM_BX_EXT + 4 * i;
    bool inside = false;
    for (int j = 0; j < nk; ++j) {
      const int* k = st + SDM_BX_KEPT + 4 * j;
      inside = inside || (raw[0] >= k[0] && raw[2] < k[0] + k[2] && raw[1] >= k[1] && raw[3] < k[1] + k[3]);
    }
    if (inside) continue;
    boxes_box(raw, H, W, margin_px, margin_pct, square, st + SDM_BX_KEPT + 4 * nk);
    ++nk;
  }
  st[SDM_BX_NKEPT] = nk;
}

// grid and loads as boxes_reduce_kernel, one slot: the extrema of R = pixels of U (root >= 0) in none of the kept boxes, into slot SDM_BX_SLOTS.
template <bool VEC>
__global__ __launch_bounds__(256) void boxes_rest_kernel(const int* __restrict__ root, int* __restrict__ state, int B, int H, int W) {
  SDM_SHARED int red[16];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int HW = H * W, chunks = (HW + SDM_ROI_PX - 1) / SDM_ROI_PX;
  const int b = blockIdx.x / chunks, base = (blockIdx.x - b * chunks) * SDM_ROI_PX;
  if (b >= B) return;
  int* st = state + b * SDM_BX_STRIDE;
  const int* pl = root + (size_t)b * HW;
  int ky0[SDM_BX_SLOTS], kx0[SDM_BX_SLOTS], ky1[SDM_BX_SLOTS], kx1[SDM_BX_SLOTS];      // (an unused slot is an empty box: all zeros)
#pragma unroll
  for (int j = 0; j < SDM_BX_SLOTS; ++j) {
    const int* k = st + SDM_BX_KEPT + 4 * j;
    ky0[j] = k[0]; kx0[j] = k[1]; ky1[j] = k[0] + k[2]; kx1[j] = k[1] + k[3];
  }
  int ymin = SDM_ROI_NONE, xmin = SDM_ROI_NONE, ymax = -1, xmax = -1;
  auto pixel = [&](int y, int x) {
    bool covered = false;
#pragma unroll
    for (int j = 0; j < SDM_BX_SLOTS; ++j) covered = covered || (y >= ky0[j] && y < ky1[j] && x >= kx0[j] && x < kx1[j]);
    if (!covered) { ymin = min(ymin, y); ymax = max(ymax, y); xmin = min(xmin, x); xmax = max(xmax, x); }
  };
  if (VEC) {
    for (int it = 0; it < 16; it += 4) {
      i32x4 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = boxes_load4(pl, base + (it + u) * 1024 + tid * 4, HW);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (v[u][0] < 0 && v[u][1] < 0 && v[u][2] < 0 && v[u][3] < 0) continue;
        const int i = base + (it + u) * 1024 + tid * 4;
        const int y = i / W, x = i - y * W;
#pragma unroll
        for (int j = 0; j < 4; ++j) if (v[u][j] >= 0) pixel(y, x + j);
      }
    }
  } else {
    for (int it = 0; it < 64; ++it) {
      const int i = base + it * 256 + tid;
      if (i < HW && pl[i] >= 0) { const int y = i / W; pixel(y, i - y * W); }
    }
  }
  if (__any(ymax >= 0)) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
      ymin = min(ymin, __shfl_xor(ymin, d)); xmin = min(xmin, __shfl_xor(xmin, d));
      ymax = max(ymax, __shfl_xor(ymax, d)); xmax = max(xmax, __shfl_xor(xmax, d));
    }
  }
  if (lane == 0) { red[wv * 4 + 0] = ymin; red[wv * 4 + 1] = xmin; red[wv * 4 + 2] = ymax; red[wv * 4 + 3] = xmax; }
  __syncthreads();
  if (tid < 4) {
    if (max(max(red[2], red[6]), max(red[10], red[14])) < 0) return;      // nothing of R in this block: no atomic
    int* dst = st + SDM_BX_EXT + SDM_BX_SLOTS * 4 + tid;
    if (tid < 2) atomicMin(dst, min(min(red[tid], red[4 + tid]), min(red[8 + tid], red[12 + tid])));
    else atomicMax((unsigned int*)dst, (unsigned int)max(max(red[tid], red[4 + tid]), max(red[8 + tid], red[12 + tid])));
  }
}

// One thread per image: boxes int32 [B][K][5] = {b, y0, x0, h, w}: the kept boxes, then box(R) if R is not empty; the whole frame if that leaves no
// entry (U is empty); {-1, 0, 0, 0, 0} in every further entry.  count (may be NULL) int32 [B].
__global__ void boxes_finalize_kernel(const int* __restrict__ state, int* __restrict__ boxes, int* __restrict__ count, int B, int H, int W, int K,
                                      int margin_px, int margin_pct, int square) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const int* st = state + b * SDM_BX_STRIDE;
  int* out = boxes + (size_t)b * K * 5;
  int n = min(st[SDM_BX_NKEPT], K - 1);      // (never more than K - 1: the rank launches fill K - 1 slots)
  for (int i = 0; i < n; ++i) {
    out[i * 5] = b;
    for (int c = 0; c < 4; ++c) out[i * 5 + 1 + c] = st[SDM_BX_KEPT + 4 * i + c];
  }
  const int* rest = st + SDM_BX_EXT + SDM_BX_SLOTS * 4;
  if (rest[0] != SDM_ROI_NONE) {
    out[n * 5] = b;
    boxes_box(rest, H, W, margin_px, margin_pct, square, out + n * 5 + 1);
    ++n;
  } else if (n == 0) {
    out[0] = b; out[1] = 0; out[2] = 0; out[3] = H; out[4] = W;
    n = 1;
  }
  for (int i = n; i < K; ++i) {
    out[i * 5] = -1;
    for (int c = 1; c < 5; ++c) out[i * 5 + c] = 0;
  }
  if (count) count[b] = n;
}

// ---- sdm_apply_matte_boxes ---------------------------------------------------------------------------------------------------------------------
// The caller's list -> the arena's: an entry that does not lie inside the planes (compared in 64 bits) becomes the void entry {-1, 0, 0, 0, 0}.
__global__ void boxes_sanitize_kernel(const int* __restrict__ in, int* __restrict__ out, int N, int B, int H, int W) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  const long long b = in[n * 5], y0 = in[n * 5 + 1], x0 = in[n * 5 + 2], h = in[n * 5 + 3], w = in[n * 5 + 4];
  const bool ok = b >= 0 && b < B && h >= 1 && w >= 1 && y0 >= 0 && x0 >= 0 && y0 + h <= H && x0 + w <= W;
  out[n * 5] = ok ? (int)b : -1;
  out[n * 5 + 1] = ok ? (int)y0 : 0; out[n * 5 + 2] = ok ? (int)x0 : 0; out[n * 5 + 3] = ok ? (int)h : 0; out[n * 5 + 4] = ok ? (int)w : 0;
}

// entry n of the sanitised list as the source of slot n: a void slot is fed the whole frame of image 0
SDM_DEV_INLINE void boxes_source(const int* __restrict__ list, int n, int H, int W, int* b, int* y0, int* x0, int* h, int* w) {
  const int* q = list + n * 5;
  if (q[0] < 0) { *b = 0; *y0 = 0; *x0 = 0; *h = H; *w = W; }
  else { *b = q[0]; *y0 = q[1]; *x0 = q[2]; *h = q[3]; *w = q[4]; }
}

// roi_prep_image_kernel over the list: image fp32 [B,H,W,3] -> NHWC16 [N,S,S,16]
__global__ void boxes_prep_image_kernel(const float* __restrict__ img, const int* __restrict__ list, void* __restrict__ out, int out_f32, int N, int H,
                                        int W, int S) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)N * S * S) return;
  const int ox = i % S, oy = (i / S) % S, n = i / ((long)S * S);
  int b, y0, x0, h, w;
  boxes_source(list, n, H, W, &b, &y0, &x0, &h, &w);
  float v[3];
  for (int c = 0; c < 3; ++c) {
    const float* pl = img + (((size_t)b * H + y0) * W + x0) * 3 + c;
    float x;
    if (h == S && w == S) x = pl[((size_t)oy * W + ox) * 3];
    else x = resize_aa_sample([&](int y, int xx) { return pl[((size_t)y * W + xx) * 3]; }, h, w, S, S, oy, ox);
    v[c] = (x - 0.5f) / 0.5f;
  }
  prep_store16(out, (size_t)i, v[0], v[1], v[2], out_f32);
}

// roi_prep_trimap_kernel over the list
__global__ void boxes_prep_trimap_kernel(const float* __restrict__ tri, const int* __restrict__ list, void* __restrict__ out, int out_f32,
                                         float* __restrict__ plane, int N, int H, int W, int S) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)N * S * S) return;
  const int ox = i % S, oy = (i / S) % S, n = i / ((long)S * S);
  int b, y0, x0, h, w;
  boxes_source(list, n, H, W, &b, &y0, &x0, &h, &w);
  const float* pl = tri + ((size_t)b * H + y0) * W + x0;
  float x;
  if (h == S && w == S) x = pl[(size_t)oy * W + ox];
  else x = resize_aa_sample([&](int y, int xx) { return pl[(size_t)y * W + xx]; }, h, w, S, S, oy, ox);
  const float t = x * 2.0f - 1.0f;
  plane[i] = t;
  prep_store16(out, (size_t)i, t, t, t, out_f32);
}

// The model's alphas [N,S,S] into the frames [B,H,W], each pixel written once: the maximum over the valid entries of its image whose box contains it of
// roi_paste_kernel's value (the clamped resize of that slot to h x w at (y0, x0)); 0.0 without one.  The values are >= 0, so 0.0 is the neutral element.
__global__ __launch_bounds__(256) void boxes_paste_kernel(const float* __restrict__ in, const int* __restrict__ list, float* __restrict__ out, int N, int B,
                                                          int H, int W, int S) {
  SDM_SHARED int q[SDM_BX_LIST * 5];
  if ((int)threadIdx.x < N * 5) q[threadIdx.x] = list[threadIdx.x];
  __syncthreads();
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)B * H * W) return;
  const int fx = i % W, fy = (i / W) % H, b = i / ((long)H * W);
  float best = 0.0f;
  for (int n = 0; n < N; ++n) {
    if (q[n * 5] != b) continue;      // (a void entry's -1 is no image)
    const int h = q[n * 5 + 3], w = q[n * 5 + 4];
    const int oy = fy - q[n * 5 + 1], ox = fx - q[n * 5 + 2];
    if (oy < 0 || oy >= h || ox < 0 || ox >= w) continue;
    const float* pl = in + (size_t)n * S * S;
    float x;
    if (h == S && w == S) x = pl[(size_t)oy * S + ox];
    else x = resize_aa_sample([&](int y, int xx) { return pl[(size_t)y * S + xx]; }, S, S, h, w, oy, ox);
    best = fmaxf(best, fminf(fmaxf(x, 0.0f), 1.0f));
  }
  out[i] = best;
}
