// k_roi.h - the subject's box and the cropped forms of the node's three resampling launches (sdm_subject_roi / sdm_apply_matte_roi in
// include/sdmatte.h; DESIGN.md 4, "matte the subject, not the frame").
//
// The box of U = { p : plane[p] > roi_threshold } is made by three launches, whatever B, H, W and the content, and never leaves the device:
//   roi_init_kernel      raw[b] = {INT_MAX, INT_MAX, 0, 0}: the neutral elements of {ymin, xmin, ymax, xmax}
//   roi_reduce_kernel    one read of the plane (4 bytes per pixel): extrema per thread, per wave (shuffles), per block (LDS), then at most four atomics per
//                        block into raw[b] - none from a block that saw no pixel of U (the background, i.e. most blocks of a photo whose subject is small)
//   roi_finalize_kernel  margins, clipping and the optional square: roi[b] = {y0, x0, h, w}, integer arithmetic only; an empty U gives the whole frame
// roi_prep_image_kernel / roi_prep_trimap_kernel / roi_paste_kernel are prep_image_kernel / prep_trimap_kernel / resize_planes_kernel (k_misc.h) with
// the box read from device memory: the same resize_aa_sample on the same values, so a call through them is bit-identical to cropping on the host,
// running the whole-frame kernels on the crop and pasting the result into zeros.
#pragma once
#include "sdm_common.h"
#include "k_misc.h"

#define SDM_ROI_PX 16384            // pixels of a block of the reduction: 256 threads x 16 vectors of 4 pixels (or 64 single pixels)
#define SDM_ROI_NONE 0x7FFFFFFF     // ymin / xmin of an image without a pixel of U

__global__ void roi_init_kernel(int* __restrict__ raw, int B) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < B * 4) raw[i] = (i & 3) < 2 ? SDM_ROI_NONE : 0;
}

// grid: B * ceil(H*W / SDM_ROI_PX) blocks of 256 threads.  VEC: 16-byte loads - W % 4 == 0 (a vector never crosses a row) and the plane 16-byte aligned.
// A pixel beyond the image reads as -1, which no threshold >= 0 lets into U.  The maxima are >= 0, so they go through the unsigned atomicMax.
template <bool VEC>
__global__ __launch_bounds__(256) void roi_reduce_kernel(const float* __restrict__ plane, int* __restrict__ raw, int B, int H, int W, float thr) {
  SDM_SHARED int red[16];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int HW = H * W, chunks = (HW + SDM_ROI_PX - 1) / SDM_ROI_PX;
  const int b = blockIdx.x / chunks, base = (blockIdx.x - b * chunks) * SDM_ROI_PX;
  const float* pl = plane + (size_t)b * HW;
  int ymin = SDM_ROI_NONE, xmin = SDM_ROI_NONE, ymax = -1, xmax = -1;
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
        const int i = base + (it + u) * 1024 + tid * 4;
        const bool m0 = v[u][0] > thr, m1 = v[u][1] > thr, m2 = v[u][2] > thr, m3 = v[u][3] > thr;
        if (m0 || m1 || m2 || m3) {
          const int y = i / W, x = i - y * W;
          ymin = min(ymin, y); ymax = max(ymax, y);
          xmin = min(xmin, x + (m0 ? 0 : m1 ? 1 : m2 ? 2 : 3));
          xmax = max(xmax, x + (m3 ? 3 : m2 ? 2 : m1 ? 1 : 0));
        }
      }
    }
  } else {
    for (int it = 0; it < 64; ++it) {
      const int i = base + it * 256 + tid;
      if (i < HW && pl[i] > thr) {
        const int y = i / W, x = i - y * W;
        ymin = min(ymin, y); ymax = max(ymax, y); xmin = min(xmin, x); xmax = max(xmax, x);
      }
    }
  }
  if (__any(ymax >= 0)) {      // wave-uniform: a wave over background skips its 24 shuffles
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
      ymin = min(ymin, __shfl_xor(ymin, s)); xmin = min(xmin, __shfl_xor(xmin, s));
      ymax = max(ymax, __shfl_xor(ymax, s)); xmax = max(xmax, __shfl_xor(xmax, s));
    }
  }
  if (lane == 0) { red[wv * 4 + 0] = ymin; red[wv * 4 + 1] = xmin; red[wv * 4 + 2] = ymax; red[wv * 4 + 3] = xmax; }
  __syncthreads();
  if (tid < 4) {
    if (max(max(red[2], red[6]), max(red[10], red[14])) < 0) return;      // no pixel of U in this block: no atomic
    int* dst = raw + b * 4 + tid;
    if (tid < 2) atomicMin(dst, min(min(red[tid], red[4 + tid]), min(red[8 + tid], red[12 + tid])));
    else atomicMax((unsigned int*)dst, (unsigned int)max(max(red[tid], red[4 + tid]), max(red[8 + tid], red[12 + tid])));
  }
}

// one axis of the box: extrema [lo, hi] of U -> {start, extent} with the margin, clipped to [0, n)
SDM_DEV_INLINE void roi_axis(int lo, int hi, int n, int margin_px, int margin_pct, int* start, int* extent) {
  const int m = margin_px + ((hi - lo + 1) * margin_pct) / 100;
  const int a = max(0, lo - m), e = min(n, hi + 1 + m);
  *start = a; *extent = e - a;
}

// ... grown to the side L of the square: half of the growth in front, shifted back into the frame, cut to the frame where the frame is shorter
SDM_DEV_INLINE void roi_square_axis(int L, int n, int* start, int* extent) {
  int a = *start - (L - *extent) / 2;
  if (a < 0) a = 0;
  if (a + L > n) a = max(0, n - L);
  *start = a; *extent = min(L, n);
}

// raw int32 [B][4] = {ymin, xmin, ymax, xmax} -> roi int32 [B][4] = {y0, x0, h, w}.  One thread per image.
__global__ void roi_finalize_kernel(const int* __restrict__ raw, int* __restrict__ roi, int B, int H, int W, int margin_px, int margin_pct, int square) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  int y0 = 0, x0 = 0, h = H, w = W;
  if (raw[b * 4] != SDM_ROI_NONE) {
    roi_axis(raw[b * 4 + 0], raw[b * 4 + 2], H, margin_px, margin_pct, &y0, &h);
    roi_axis(raw[b * 4 + 1], raw[b * 4 + 3], W, margin_px, margin_pct, &x0, &w);
    if (square) {
      const int L = max(h, w);      // (the longer axis keeps its start and extent: its growth is 0)
      roi_square_axis(L, H, &y0, &h);
      roi_square_axis(L, W, &x0, &w);
    }
  }
  roi[b * 4 + 0] = y0; roi[b * 4 + 1] = x0; roi[b * 4 + 2] = h; roi[b * 4 + 3] = w;
}

// prep_image_kernel on the box of every image: image fp32 [B,H,W,3] -> NHWC16 [B,S,S,16] of the h x w pixels at (y0, x0)
__global__ void roi_prep_image_kernel(const float* __restrict__ img, const int* __restrict__ roi, void* __restrict__ out, int out_f32, int B, int H, int W,
                                      int S) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)B * S * S) return;
  const int ox = i % S, oy = (i / S) % S, b = i / ((long)S * S);
  const int y0 = roi[b * 4 + 0], x0 = roi[b * 4 + 1], h = roi[b * 4 + 2], w = roi[b * 4 + 3];
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

// prep_trimap_kernel on the box of every image
__global__ void roi_prep_trimap_kernel(const float* __restrict__ tri, const int* __restrict__ roi, void* __restrict__ out, int out_f32,
                                       float* __restrict__ plane, int B, int H, int W, int S) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)B * S * S) return;
  const int ox = i % S, oy = (i / S) % S, b = i / ((long)S * S);
  const int y0 = roi[b * 4 + 0], x0 = roi[b * 4 + 1], h = roi[b * 4 + 2], w = roi[b * 4 + 3];
  const float* pl = tri + ((size_t)b * H + y0) * W + x0;
  float x;
  if (h == S && w == S) x = pl[(size_t)oy * W + ox];
  else x = resize_aa_sample([&](int y, int xx) { return pl[(size_t)y * W + xx]; }, h, w, S, S, oy, ox);
  const float t = x * 2.0f - 1.0f;
  plane[i] = t;
  prep_store16(out, (size_t)i, t, t, t, out_f32);
}

// the model's alpha [B,S,S] back into the frame [B,H,W]: resize_planes_kernel (clamped) to h x w at (y0, x0), 0.0 outside the box
__global__ void roi_paste_kernel(const float* __restrict__ in, const int* __restrict__ roi, float* __restrict__ out, int B, int H, int W, int S) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)B * H * W) return;
  const int fx = i % W, fy = (i / W) % H, b = i / ((long)H * W);
  const int y0 = roi[b * 4 + 0], x0 = roi[b * 4 + 1], h = roi[b * 4 + 2], w = roi[b * 4 + 3];
  const int oy = fy - y0, ox = fx - x0;
  float x = 0.0f;
  if (oy >= 0 && oy < h && ox >= 0 && ox < w) {
    const float* pl = in + (size_t)b * S * S;
    if (h == S && w == S) x = pl[(size_t)oy * S + ox];
    else x = resize_aa_sample([&](int y, int xx) { return pl[(size_t)y * S + xx]; }, S, S, h, w, oy, ox);
    x = fminf(fmaxf(x, 0.0f), 1.0f);
  }
  out[i] = x;
}
