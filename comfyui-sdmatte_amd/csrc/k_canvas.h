// k_canvas.h - the cut-out on a canvas (sdm_compose_canvas in include/sdmatte.h, which is the normative text; DESIGN.md 4, "frame the cut-out").
//
// The box of the alpha comes from op_roi_box (k_roi.h: roi_init, roi_reduce, roi_finalize) and never leaves the device; the canvas size is known on the host.
//   canvas_fit_kernel           roi {y0, x0, h, w} -> placement {y0, x0, h, w, dy0, dx0, dh, dw}: integers only, one thread per image
//   canvas_layer_px()           the premultiplied subject layer (a F.r, a F.g, a F.b, a) at one canvas pixel: resize_aa_sample (k_misc.h) of the four planes
//                               of the box from (h, w) to (dh, dw), the plain copy when the sizes are equal, 0 outside the destination rectangle.  The box is
//                               read from device memory by every thread, as in roi_prep_image_kernel.
// Without a shadow ONE more launch writes the canvas, and no canvas-sized intermediate exists:
//   canvas_compose_kernel<CHN>  layer over background per pixel; CHN = 4: one pixel and one 16-byte store per thread; CHN = 3: a run of 4 pixels of the flat
//                               [B canvas_h canvas_w] index and 3 x 16-byte stores per thread (as gf_apply_kernel)
// With a shadow THREE launches:
//   canvas_place_kernel         layer -> plane [B][canvas_h][canvas_w][4], one 16-byte store per thread
//   canvas_blur_rows_kernel     T(y, x) = sum over i = -r .. r (ascending) of w_i A_s(y, x - shadow_dx + i), 0 beyond the canvas.  A block owns 256 columns of
//                               one row: the 256 + 2r alphas go through LDS once, every thread sums its 2r + 1 neighbours out of LDS.
//   canvas_blur_compose_kernel<CHN>  S(y, x) = opacity * sum over j = -r .. r (ascending) of w_j T(y - shadow_dy + j, x), rows beyond the canvas 0, then the
//                               composition.  A block owns 64 columns x canvas_tile_h(r) rows: the tile of T with its halo of r rows goes through LDS once, the
//                               column sums go back to LDS, and the composition reads them in the store pattern of canvas_compose_kernel (CHN = 3: runs of 4
//                               pixels of one row).
// The weights come by value (CanvasBlur): they are wave-uniform and indexed by the loop counter.  Integer and compare logic is plain C++: the emulator
// build (SDM_EMU) runs this source.
#pragma once
#include "sdm_common.h"
#include "k_misc.h"
#include "k_guided.h"

#define SDM_CANVAS_R 96                  // SDM_CANVAS_MAX_SHADOW_RADIUS (include/sdmatte.h)
#define SDM_CANVAS_ROW_W 256             // columns of a block of canvas_blur_rows_kernel
#define SDM_CANVAS_TW 64                 // tile columns of canvas_blur_compose_kernel
#define SDM_CANVAS_TH 32                 // tile rows at r <= 92
#define SDM_CANVAS_RR 216                // LDS rows of T: tile rows + 2r (r = 96 leaves 24 tile rows)

struct CanvasBlur { int r; float w[2 * SDM_CANVAS_R + 1]; };      // w[k] = weight of offset k - r, k = 0 .. 2r

SDM_HD_INLINE int canvas_tile_h(int r) { return SDM_CANVAS_RR - 2 * r < SDM_CANVAS_TH ? SDM_CANVAS_RR - 2 * r : SDM_CANVAS_TH; }
// dynamic LDS of canvas_blur_compose_kernel: (tile rows + 2r) x 64 floats of T, then SDM_CANVAS_TH x 64 floats of S (both offsets multiples of 256 bytes)
SDM_HD_INLINE size_t canvas_blur_smem(int r) { return (size_t)(canvas_tile_h(r) + 2 * r + SDM_CANVAS_TH) * SDM_CANVAS_TW * 4; }

// roi int32 [B][4] -> place int32 [B][8] (and place2, the caller's copy, unless null).  One thread per image; the products are 64-bit.
__global__ void canvas_fit_kernel(const int* __restrict__ roi, int* __restrict__ place, int* __restrict__ place2, int B, int canvas_h, int canvas_w,
                                  int fill_pct, int valign) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const long long h = roi[b * 4 + 2], w = roi[b * 4 + 3];
  const long long ch = canvas_h, cw = canvas_w;
  long long th = ch * fill_pct / 100, tw = cw * fill_pct / 100;
  if (th < 1) th = 1;
  if (tw < 1) tw = 1;
  long long dh, dw;
  if (th * w <= tw * h) { dh = th; dw = (w * th + h / 2) / h; if (dw < 1) dw = 1; }
  else { dw = tw; dh = (h * tw + w / 2) / w; if (dh < 1) dh = 1; }
  const long long mv = (ch - th) / 2;
  const long long dy0 = valign == 0 ? mv : (valign == 1 ? (ch - dh) / 2 : ch - mv - dh);
  const int v[8] = {roi[b * 4 + 0], roi[b * 4 + 1], (int)h, (int)w, (int)dy0, (int)((cw - dw) / 2), (int)dh, (int)dw};
  for (int k = 0; k < 8; ++k) {
    place[b * 8 + k] = v[k];
    if (place2) place2[b * 8 + k] = v[k];
  }
}

// the subject layer (P_s, A_s) of image b at canvas pixel (cy, cx); pl = place + 8 b
SDM_DEV_INLINE f32x4 canvas_layer_px(const float* __restrict__ fg, const float* __restrict__ alpha, const int* __restrict__ pl, int H, int W, int b, int cy,
                                     int cx) {
  const int y0 = pl[0], x0 = pl[1], h = pl[2], w = pl[3], dh = pl[6], dw = pl[7];
  const int oy = cy - pl[4], ox = cx - pl[5];
  f32x4 r = {0.0f, 0.0f, 0.0f, 0.0f};
  if (oy < 0 || oy >= dh || ox < 0 || ox >= dw) return r;
  const float* ap = alpha + ((size_t)b * H + y0) * W + x0;
  const float* fp = fg + (((size_t)b * H + y0) * W + x0) * 3;
  if (dh == h && dw == w) {
    const size_t i = (size_t)oy * W + ox;
    const float a = gf_alpha(ap[i]);
    r[0] = a * fp[i * 3]; r[1] = a * fp[i * 3 + 1]; r[2] = a * fp[i * 3 + 2]; r[3] = a;
    return r;
  }
#pragma unroll
  for (int c = 0; c < 3; ++c)
    r[c] = resize_aa_sample([&](int y, int xx) { const size_t i = (size_t)y * W + xx; return gf_alpha(ap[i]) * fp[i * 3 + c]; }, h, w, dh, dw, oy, ox);
  r[3] = resize_aa_sample([&](int y, int xx) { return gf_alpha(ap[(size_t)y * W + xx]); }, h, w, dh, dw, oy, ox);
  return r;
}

// the opaque background of canvas pixel (y, x) of image b (bg_mode 1: the colour; 2: the image, one for the batch or one per image); 0 without one
struct CanvasBg { int mode; float rgb[3]; const float* image; int batch; };
SDM_DEV_INLINE void canvas_bg_px(const CanvasBg& bg, int canvas_h, int canvas_w, int b, int y, int x, float (&c)[3]) {
  c[0] = c[1] = c[2] = 0.0f;
  if (bg.mode == 1) { c[0] = bg.rgb[0]; c[1] = bg.rgb[1]; c[2] = bg.rgb[2]; }
  else if (bg.mode == 2) {
    const float* p = bg.image + (((size_t)(bg.batch == 1 ? 0 : b) * canvas_h + y) * canvas_w + x) * 3;
    c[0] = p[0]; c[1] = p[1]; c[2] = p[2];
  }
}

// "over" from bottom to top: background (c, 1) or nothing, shadow (0, S), subject L = (P_s, A_s).  The alpha over an opaque background is 1.0 by definition.
SDM_DEV_INLINE f32x4 canvas_over(f32x4 L, float S, int bg_mode, const float (&c)[3]) {
  const float t = 1.0f - S, k = 1.0f - L[3];
  f32x4 r;
  r[0] = L[0] + k * (t * c[0]); r[1] = L[1] + k * (t * c[1]); r[2] = L[2] + k * (t * c[2]);
  r[3] = bg_mode ? 1.0f : L[3] + k * S;
  return r;
}

// n <= 4 consecutive pixels from flat pixel index p on: CHN = 3 the premultiplied P; CHN = 4 straight RGBA (P / A where A > 0, else 0; A).
// vec: out is 16-byte aligned (and p % 4 == 0 for CHN = 3); a shorter run goes value by value.
template <int CHN>
SDM_DEV_INLINE void canvas_store(float* __restrict__ out, size_t p, int n, const f32x4 (&res)[4], bool vec) {
  if (CHN == 4) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (k < n) {
        const float A = res[k][3];
        f32x4 o = {0.0f, 0.0f, 0.0f, A};
        if (A > 0.0f) { o[0] = res[k][0] / A; o[1] = res[k][1] / A; o[2] = res[k][2] / A; }
        float* d = out + (p + k) * 4;
        if (vec) *(f32x4*)d = o;
        else { d[0] = o[0]; d[1] = o[1]; d[2] = o[2]; d[3] = o[3]; }
      }
    }
  } else {
    float* d = out + p * 3;
    if (vec && n == 4) {
      f32x4 o0 = {res[0][0], res[0][1], res[0][2], res[1][0]}, o1 = {res[1][1], res[1][2], res[2][0], res[2][1]},
            o2 = {res[2][2], res[3][0], res[3][1], res[3][2]};
      ((f32x4*)d)[0] = o0; ((f32x4*)d)[1] = o1; ((f32x4*)d)[2] = o2;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (k < n) { d[k * 3] = res[k][0]; d[k * 3 + 1] = res[k][1]; d[k * 3 + 2] = res[k][2]; }
    }
  }
}

// no shadow: place and compose in one pass.  grid: ceil(ceil(B canvas_h canvas_w / PX) / 256) blocks of 256 threads, PX = 1 (CHN = 4) or 4 (CHN = 3) pixels
// of the flat index per thread (a run may cross the end of a row or of an image).  vec: out is 16-byte aligned.
template <int CHN>
__global__ __launch_bounds__(256) void canvas_compose_kernel(const float* __restrict__ fg, const float* __restrict__ alpha, const int* __restrict__ place, int B,
                                                             int H, int W, int canvas_h, int canvas_w, CanvasBg bg, int vec, float* __restrict__ out) {
  constexpr int PX = CHN == 4 ? 1 : 4;
  const int total = B * canvas_h * canvas_w;
  const int t = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (t >= (total + PX - 1) / PX) return;
  const int g0 = t * PX, n = min(PX, total - g0);
  int x = g0 % canvas_w, y = (g0 / canvas_w) % canvas_h, b = g0 / (canvas_w * canvas_h);
  f32x4 res[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    res[k][0] = res[k][1] = res[k][2] = res[k][3] = 0.0f;
    if (k < n) {
      float c[3];
      canvas_bg_px(bg, canvas_h, canvas_w, b, y, x, c);
      res[k] = canvas_over(canvas_layer_px(fg, alpha, place + b * 8, H, W, b, y, x), 0.0f, bg.mode, c);
      if (++x == canvas_w) { x = 0; if (++y == canvas_h) { y = 0; ++b; } }
    }
  }
  canvas_store<CHN>(out, (size_t)g0, n, res, vec != 0);
}

// with a shadow: the layer as a plane [B][canvas_h][canvas_w][4].  grid: ceil(B canvas_h canvas_w / 256) blocks of 256 threads.
__global__ __launch_bounds__(256) void canvas_place_kernel(const float* __restrict__ fg, const float* __restrict__ alpha, const int* __restrict__ place, int B,
                                                           int H, int W, int canvas_h, int canvas_w, float* __restrict__ layer) {
  const int total = B * canvas_h * canvas_w;
  const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (i >= total) return;
  const int x = i % canvas_w, y = (i / canvas_w) % canvas_h, b = i / (canvas_w * canvas_h);
  ((f32x4*)layer)[i] = canvas_layer_px(fg, alpha, place + b * 8, H, W, b, y, x);
}

// grid: B * canvas_h * ceil(canvas_w / 256) blocks of 256 threads.  layer: [B][canvas_h][canvas_w][4] (A_s is channel 3); tplane: [B][canvas_h][canvas_w].
__global__ __launch_bounds__(256) void canvas_blur_rows_kernel(const float* __restrict__ layer, int B, int canvas_h, int canvas_w, int shadow_dx,
                                                               CanvasBlur blur, float* __restrict__ tplane) {
  SDM_SHARED float as[SDM_CANVAS_ROW_W + 2 * SDM_CANVAS_R];
  const int tid = threadIdx.x, r = blur.r;
  const int nbx = (canvas_w + SDM_CANVAS_ROW_W - 1) / SDM_CANVAS_ROW_W;
  const int blk = blockIdx.x;
  const int row = blk / nbx, x0 = (blk - row * nbx) * SDM_CANVAS_ROW_W;      // row = b * canvas_h + y
  if (row >= B * canvas_h) return;
  const float* lp = layer + (size_t)row * canvas_w * 4;
  for (int idx = tid; idx < SDM_CANVAS_ROW_W + 2 * r; idx += 256) {
    const int xs = x0 - shadow_dx - r + idx;
    as[idx] = (xs >= 0 && xs < canvas_w) ? lp[(size_t)xs * 4 + 3] : 0.0f;
  }
  __syncthreads();
  const int x = x0 + tid;
  if (x < canvas_w) {
    float s = 0.0f;
    for (int k = 0; k <= 2 * r; ++k) s += blur.w[k] * as[tid + k];
    tplane[(size_t)row * canvas_w + x] = s;
  }
}

// grid: B * ceil(canvas_h / canvas_tile_h(r)) * ceil(canvas_w / 64) blocks of 256 threads, canvas_blur_smem(r) bytes of dynamic LDS.
// vec: out is 16-byte aligned, and canvas_w % 4 == 0 for CHN = 3 (a run of 4 pixels of a row then starts at a multiple of 4 pixels).
template <int CHN>
__global__ __launch_bounds__(256) void canvas_blur_compose_kernel(const float* __restrict__ layer, const float* __restrict__ tplane, int B, int canvas_h,
                                                                  int canvas_w, int shadow_dy, float opacity, CanvasBlur blur, CanvasBg bg, int vec,
                                                                  float* __restrict__ out) {
  SDM_DYN_SMEM(smem);
  const int tid = threadIdx.x, r = blur.r, th = canvas_tile_h(r);
  float* ts = (float*)smem;                                       // [th + 2r][64]: T of rows y0 - shadow_dy - r ..
  float* ss = ts + (size_t)(th + 2 * r) * SDM_CANVAS_TW;          // [th][64]: S of the tile
  const int nbx = (canvas_w + SDM_CANVAS_TW - 1) / SDM_CANVAS_TW, nby = (canvas_h + th - 1) / th;
  const int blk = blockIdx.x;
  const int b = blk / (nbx * nby), y0 = ((blk / nbx) % nby) * th, x0 = (blk % nbx) * SDM_CANVAS_TW;
  if (b >= B) return;
  const float* tp = tplane + (size_t)b * canvas_h * canvas_w;
  for (int idx = tid; idx < (th + 2 * r) * SDM_CANVAS_TW; idx += 256) {
    const int ys = y0 - shadow_dy - r + (idx >> 6), x = x0 + (idx & 63);
    ts[idx] = (ys >= 0 && ys < canvas_h && x < canvas_w) ? tp[(size_t)ys * canvas_w + x] : 0.0f;
  }
  __syncthreads();
  for (int idx = tid; idx < th * SDM_CANVAS_TW; idx += 256) {
    const float* col = ts + idx;                                  // row (idx >> 6) + k of the region, the thread's column
    float s = 0.0f;
    for (int k = 0; k <= 2 * r; ++k) s += blur.w[k] * col[k * SDM_CANVAS_TW];
    ss[idx] = opacity * s;
  }
  __syncthreads();
  constexpr int PX = CHN == 4 ? 1 : 4, RUNS = SDM_CANVAS_TW / PX;
  for (int idx = tid; idx < th * RUNS; idx += 256) {
    const int ry = idx / RUNS, cx = (idx - ry * RUNS) * PX;
    const int y = y0 + ry, x = x0 + cx;
    const int n = min(PX, canvas_w - x);
    if (y >= canvas_h || n <= 0) continue;
    const size_t p = ((size_t)b * canvas_h + y) * canvas_w + x;
    f32x4 res[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      res[k][0] = res[k][1] = res[k][2] = res[k][3] = 0.0f;
      if (k < n) {
        float c[3];
        canvas_bg_px(bg, canvas_h, canvas_w, b, y, x + k, c);
        res[k] = canvas_over(((const f32x4*)layer)[p + k], ss[ry * SDM_CANVAS_TW + cx + k], bg.mode, c);
      }
    }
    canvas_store<CHN>(out, p, n, res, vec != 0);
  }
}
