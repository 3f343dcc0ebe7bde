// k_plate.h - the photo without its subject: push-pull fill of the subject's hole (sdm_fill_background; DESIGN.md 4, "clean plate").
//
//   a  = clamp01(alpha, NaN -> 0), a = max(a, clamp01(hole, NaN -> 0)) with a hole plane;  C = bg or image;  w_0 = clamp(1 - a / alpha_cut, 0, 1)
//   levels  (h_l, w_l) = (ceil(H / 2^l), ceil(W / 2^l)), level 0 the photo, down to (1, 1)
//   pull    a pixel of level l + 1 has the children (2 i + dy, 2 j + dx) that exist at level l, taken in the order (0,0) (0,1) (1,0) (1,1):
//           Sw = sum w, Sc = sum w C;  C_{l+1} = Sw > 0 ? Sc / Sw : 0;  w_{l+1} = min(1, Sw)
//   push    F_top = C_top;  n = y >> 1, f = clamp(n + (y odd ? 1 : -1)) per axis;
//           U = 0.75 (0.75 F[ny,nx] + 0.25 F[ny,fx]) + 0.25 (0.75 F[fy,nx] + 0.25 F[fy,fx]);  F_l = w_l C_l + (1 - w_l) U;  out = F_0
// fp32, true divisions, no contraction.  A child that does not exist enters the sums as (C, w) = (0, 0): x + 0 == x, so leaving it out and adding it agree
// (to the sign of a zero).
//
// A level l >= 1 is a plane of 16 bytes per pixel [C.r C.g C.b w] in the arena; the push overwrites C by F in place (a pixel's (C, w) is read by the one
// block that writes its F, in the same launch; the coarser levels a launch reads are not written by it).  S = the number of levels with
// max(h_l, w_l) > 32.  THREE kernels, 1 + 2 ceil(S / 3) launches:
//   plate_pull   a block of 256 threads owns a tile of 64 x 32 pixels of level l (the inputs when l = 0, else the plane) and reduces it through up to
//                three levels: a thread's 4 x 2 pixels give two pixels of level l + 1, which cross LDS for the 16 x 8 of level l + 2 and the 8 x 4 of level
//                l + 3.  Tiles are even and aligned, so a pull never leaves its tile: no halo.  Launches at l = 0, 3, 6, ... while l < S.
//   plate_small  one block of 1024 threads per image holds level S (at most 32 x 32) and every coarser level in LDS (1365 pixels), pulls up to (1, 1) and
//                pushes back down to level S.  With S = 0 it reads the inputs and writes `out`: the whole call is this launch.
//   plate_push   a block owns a tile of 64 x 32 pixels of its finest level lf and expands through up to three levels in LDS.  A pixel of level j reads
//                rows (y >> 1) and (y >> 1) +- 1 of level j + 1, so the region of level lf + j is the tile >> j plus a halo of ONE pixel at every level
//                (6 x 10, 10 x 18, 18 x 34).  The levels in between are computed in LDS from their (C, w) planes and never stored; the finest goes to
//                memory.  The last push reads image / alpha (/ bg / hole) and writes `out`.  The first push takes the S mod 3 levels left over, the
//                others three each.
// Level-0 accesses: a thread owns a run of 4 pixels (ts_load: 3 x 16 + 16 bytes when the tensors are 16-byte aligned and W % 4 == 0, scalar otherwise, one
// arithmetic path).  No load leaves the planes: every global index is checked against its level's size, a region slot outside its level is never read
// (n lies in the level because y does, f is clamped into it), and every LDS index lies in its region (see plate_up).
#pragma once
#include "sdm_common.h"
#include "k_guided.h"      // gf_alpha
#include "k_temporal.h"    // ts_load

#define SDM_PLATE_SMALL 32                                              // a level is small iff max(h, w) <= SDM_PLATE_SMALL
#define SDM_PLATE_SMALL_PX 1024                                         // = SDM_PLATE_SMALL^2: threads of plate_small_kernel
#define SDM_PLATE_SMALL_LDS 1365                                        // 1024 + 256 + 64 + 16 + 4 + 1 pixels: the small levels of one image
#define SDM_PLATE_GROUP 3                                               // levels per pull / push launch
#define SDM_PLATE_TW 64                                                 // tile of the finest level of a launch
#define SDM_PLATE_TH 32

SDM_HD_INLINE int plate_dim(int n, int l) { return (n + (1 << l) - 1) >> l; }      // ceil(n / 2^l) = l times ceil(. / 2); n <= 32768, l <= 15

// the level-0 planes of a call.  vec: W % 4 == 0 and C, alpha, hole (if any) and out 16-byte aligned
struct PlateIn { const float* C; const float* alpha; const float* hole; float cut; int vec; };

SDM_DEV_INLINE float plate_w0(float alpha, float hole, float cut) {
#pragma clang fp contract(off)
  const float a = fmaxf(gf_alpha(alpha), gf_alpha(hole));
  return fminf(fmaxf(1.0f - a / cut, 0.0f), 1.0f);
}

// a run of up to 4 pixels of level 0 as [C.rgb, w0]; pixels i >= npx do not exist and read as zeros.  g: pixel index of the run's first pixel
SDM_DEV_INLINE void plate_load0(const PlateIn& in, size_t g, int npx, f32x4 (&p)[4]) {
  float c[12], a[4] = {1.0f, 1.0f, 1.0f, 1.0f}, hl[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int i = 0; i < 12; ++i) c[i] = 0.0f;
  if (npx > 0) {
    ts_load(in.C, in.alpha, g, npx, in.vec != 0, true, c, a);
    if (in.hole) {
      if (in.vec) {
        const f32x4 hv = *(const f32x4*)(in.hole + g);
#pragma unroll
        for (int i = 0; i < 4; ++i) hl[i] = hv[i];
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (i < npx) hl[i] = in.hole[g + i];
      }
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    p[i] = f32x4{c[3 * i], c[3 * i + 1], c[3 * i + 2], plate_w0(a[i], hl[i], in.cut)};
    if (i >= npx) p[i] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  }
}

// one pixel of the next level from its children (0,0) (0,1) (1,0) (1,1); an absent child is (0, 0, 0, 0)
SDM_DEV_INLINE f32x4 plate_reduce(const f32x4 t0, const f32x4 t1, const f32x4 t2, const f32x4 t3) {
#pragma clang fp contract(off)
  const float sw = ((t0[3] + t1[3]) + t2[3]) + t3[3];
  f32x4 r;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float sc = ((t0[3] * t0[k] + t1[3] * t1[k]) + t2[3] * t2[k]) + t3[3] * t3[k];
    r[k] = sw > 0.0f ? sc / sw : 0.0f;
  }
  r[3] = fminf(1.0f, sw);
  return r;
}

// F of pixel (y, x) from its own cw = [C.rgb, w] and the F of the coarser level (hc x wc), held in `nb` as the rows oy .. and columns ox .. of that level
// at `pitch`.  ny = y >> 1 < hc because y lies in its level; fy is clamped into [0, hc): the four reads lie in the coarser level, and in the caller's
// region by the halo argument in the header.  The result keeps w in [3].
SDM_DEV_INLINE f32x4 plate_up(const f32x4* nb, int pitch, int oy, int ox, int hc, int wc, int y, int x, const f32x4 cw) {
#pragma clang fp contract(off)
  const int ny = y >> 1, nx = x >> 1;
  const int fy = min(max(ny + ((y & 1) ? 1 : -1), 0), hc - 1), fx = min(max(nx + ((x & 1) ? 1 : -1), 0), wc - 1);
  const f32x4 a = nb[(ny - oy) * pitch + (nx - ox)], b = nb[(ny - oy) * pitch + (fx - ox)];
  const f32x4 c = nb[(fy - oy) * pitch + (nx - ox)], d = nb[(fy - oy) * pitch + (fx - ox)];
  f32x4 r;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float u = 0.75f * (0.75f * a[k] + 0.25f * b[k]) + 0.25f * (0.75f * c[k] + 0.25f * d[k]);
    r[k] = cw[3] * cw[k] + (1.0f - cw[3]) * u;
  }
  r[3] = cw[3];
  return r;
}

// grid: B * ceil(h / 32) * ceil(w / 64) blocks of 256 threads, (h, w) = level l.  src = the plane of level l (unused when l == 0: the inputs);
// d1, d2, d3 = the planes of levels l + 1 .. l + n, n in 1 .. 3.
__global__ __launch_bounds__(256) void plate_pull_kernel(PlateIn in, const f32x4* __restrict__ src, int B, int H, int W, int l, int n,
                                                         f32x4* __restrict__ d1, f32x4* __restrict__ d2, f32x4* __restrict__ d3) {
  SDM_SHARED f32x4 s1[(SDM_PLATE_TH / 2) * (SDM_PLATE_TW / 2)];
  SDM_SHARED f32x4 s2[(SDM_PLATE_TH / 4) * (SDM_PLATE_TW / 4)];
  const int tid = threadIdx.x;
  const int h = plate_dim(H, l), w = plate_dim(W, l);
  const int nbx = (w + SDM_PLATE_TW - 1) / SDM_PLATE_TW, nby = (h + SDM_PLATE_TH - 1) / SDM_PLATE_TH;
  const int blk = blockIdx.x;
  const int b = blk / (nbx * nby), by = (blk / nbx) % nby, bx = blk % nbx;
  if (b >= B) return;
  {
    const int tx = tid & 15, ty = tid >> 4;
    const int y = by * SDM_PLATE_TH + 2 * ty, x = bx * SDM_PLATE_TW + 4 * tx;
    f32x4 p[2][4];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const int npx = y + r < h ? max(0, min(4, w - x)) : 0;
      if (l == 0) {
        plate_load0(in, ((size_t)b * h + (y + r)) * w + x, npx, p[r]);
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) p[r][i] = i < npx ? src[((size_t)b * h + (y + r)) * w + x + i] : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
      }
    }
    const int h1 = plate_dim(H, l + 1), w1 = plate_dim(W, l + 1);
    const int y1 = by * (SDM_PLATE_TH / 2) + ty;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const f32x4 q = plate_reduce(p[0][2 * k], p[0][2 * k + 1], p[1][2 * k], p[1][2 * k + 1]);
      const int x1 = bx * (SDM_PLATE_TW / 2) + 2 * tx + k;
      s1[ty * (SDM_PLATE_TW / 2) + 2 * tx + k] = q;                     // (a pixel that does not exist is all zeros: it has no children)
      if (y1 < h1 && x1 < w1) d1[((size_t)b * h1 + y1) * w1 + x1] = q;
    }
  }
  if (n >= 2) {                                                         // (n is the same for the whole grid)
    __syncthreads();
    if (tid < (SDM_PLATE_TH / 4) * (SDM_PLATE_TW / 4)) {
      const int px = tid & 15, py = tid >> 4;
      const f32x4* c = s1 + (2 * py) * (SDM_PLATE_TW / 2) + 2 * px;
      const f32x4 q = plate_reduce(c[0], c[1], c[SDM_PLATE_TW / 2], c[SDM_PLATE_TW / 2 + 1]);
      const int h2 = plate_dim(H, l + 2), w2 = plate_dim(W, l + 2);
      const int y2 = by * (SDM_PLATE_TH / 4) + py, x2 = bx * (SDM_PLATE_TW / 4) + px;
      s2[tid] = q;
      if (y2 < h2 && x2 < w2) d2[((size_t)b * h2 + y2) * w2 + x2] = q;
    }
  }
  if (n >= 3) {
    __syncthreads();
    if (tid < (SDM_PLATE_TH / 8) * (SDM_PLATE_TW / 8)) {
      const int px = tid & 7, py = tid >> 3;
      const f32x4* c = s2 + (2 * py) * (SDM_PLATE_TW / 4) + 2 * px;
      const f32x4 q = plate_reduce(c[0], c[1], c[SDM_PLATE_TW / 4], c[SDM_PLATE_TW / 4 + 1]);
      const int h3 = plate_dim(H, l + 3), w3 = plate_dim(W, l + 3);
      const int y3 = by * (SDM_PLATE_TH / 8) + py, x3 = bx * (SDM_PLATE_TW / 8) + px;
      if (y3 < h3 && x3 < w3) d3[((size_t)b * h3 + y3) * w3 + x3] = q;
    }
  }
}

// grid: B blocks of 1024 threads.  S = the first small level, (hs, ws) <= 32 x 32.  S > 0: lv = the plane of level S, (C, w) in and F out, in place.
// S == 0: the inputs in, `out` out (scalar accesses: at most 1024 pixels per image).
__global__ __launch_bounds__(SDM_PLATE_SMALL_PX) void plate_small_kernel(PlateIn in, f32x4* __restrict__ lv, int B, int H, int W, int S,
                                                                         float* __restrict__ out) {
  SDM_SHARED f32x4 sp[SDM_PLATE_SMALL_LDS];
  const int tid = threadIdx.x, b = blockIdx.x;
  if (b >= B) return;
  const int hs = plate_dim(H, S), ws = plate_dim(W, S);
  const size_t pix = (size_t)b * hs * ws + tid;
  if (tid < hs * ws) {
    if (S == 0) {
      const float hl = in.hole ? in.hole[pix] : 0.0f;
      sp[tid] = f32x4{in.C[pix * 3], in.C[pix * 3 + 1], in.C[pix * 3 + 2], plate_w0(in.alpha[pix], hl, in.cut)};
    } else {
      sp[tid] = lv[pix];
    }
  }
  // pull: level k of the block (level S + k of the image) starts at off_k = sum over j < k of (32 >> j)^2 and has the pitch of its own width; its
  // sides are at most 32 >> k, so it ends before off_{k+1}
  int top = 0;
  {
    int off = 0;
    for (int k = 0, hk = hs, wk = ws; hk > 1 || wk > 1; ++k) {
      const int hn = (hk + 1) >> 1, wn = (wk + 1) >> 1, offn = off + (SDM_PLATE_SMALL >> k) * (SDM_PLATE_SMALL >> k);
      __syncthreads();
      if (tid < hn * wn) {
        const int y = tid / wn, x = tid - y * wn;
        const f32x4 z = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        const bool ry = 2 * y + 1 < hk, rx = 2 * x + 1 < wk;
        const f32x4* c = sp + off + (2 * y) * wk + 2 * x;
        sp[offn + tid] = plate_reduce(c[0], rx ? c[1] : z, ry ? c[wk] : z, (ry && rx) ? c[wk + 1] : z);
      }
      hk = hn; wk = wn; off = offn; top = k + 1;
    }
  }
  // push: F_top = C_top; level k from level k + 1, in place (a thread rewrites its own pixel and reads the coarser level only)
  for (int k = top - 1; k >= 0; --k) {
    int off = 0;
    for (int j = 0; j < k; ++j) off += (SDM_PLATE_SMALL >> j) * (SDM_PLATE_SMALL >> j);
    const int offc = off + (SDM_PLATE_SMALL >> k) * (SDM_PLATE_SMALL >> k);
    const int hk = plate_dim(hs, k), wk = plate_dim(ws, k), hc = plate_dim(hs, k + 1), wc = plate_dim(ws, k + 1);
    __syncthreads();
    if (tid < hk * wk) {
      const int y = tid / wk, x = tid - y * wk;
      sp[off + tid] = plate_up(sp + offc, wc, 0, 0, hc, wc, y, x, sp[off + tid]);
    }
  }
  if (tid < hs * ws) {                                                  // (a thread reads back the pixel it wrote itself)
    const f32x4 f = sp[tid];
    if (S == 0) { out[pix * 3] = f[0]; out[pix * 3 + 1] = f[1]; out[pix * 3 + 2] = f[2]; }
    else lv[pix] = f;
  }
}

// grid: B * ceil(hf / 32) * ceil(wf / 64) blocks of 256 threads, (hf, wf) = level lf, the finest of this launch.  n in 1 .. 3: `coarse` = the plane of
// level lf + n with F in it; m2 / m1 = the planes of levels lf + 2 / lf + 1 where these lie below lf + n ((C, w), read only); fine = the plane of level
// lf, (C, w) in and F out in place - or, when lf == 0, the inputs in and `out` out.
__global__ __launch_bounds__(256) void plate_push_kernel(PlateIn in, const f32x4* __restrict__ coarse, const f32x4* __restrict__ m2,
                                                         const f32x4* __restrict__ m1, f32x4* __restrict__ fine, int B, int H, int W, int lf, int n,
                                                         float* __restrict__ out) {
  SDM_SHARED f32x4 r1[(SDM_PLATE_TH / 2 + 2) * (SDM_PLATE_TW / 2 + 2)];
  SDM_SHARED f32x4 r2[(SDM_PLATE_TH / 4 + 2) * (SDM_PLATE_TW / 4 + 2)];
  SDM_SHARED f32x4 r3[(SDM_PLATE_TH / 8 + 2) * (SDM_PLATE_TW / 8 + 2)];
  const int tid = threadIdx.x;
  const int hf = plate_dim(H, lf), wf = plate_dim(W, lf);
  const int nbx = (wf + SDM_PLATE_TW - 1) / SDM_PLATE_TW, nby = (hf + SDM_PLATE_TH - 1) / SDM_PLATE_TH;
  const int blk = blockIdx.x;
  const int b = blk / (nbx * nby), by = blk / nbx % nby, bx = blk % nbx;
  if (b >= B) return;
  // the region of level lf + j: rows by (32 >> j) - 1 .. by (32 >> j) + (32 >> j), columns likewise: (32 >> j) + 2 by (64 >> j) + 2 slots
  for (int j = n; j >= 1; --j) {
    f32x4* reg = j == 1 ? r1 : j == 2 ? r2 : r3;
    const f32x4* nb = j == 1 ? r2 : r3;                                 // the region of level lf + j + 1 (not read when j == n)
    const int rh = (SDM_PLATE_TH >> j) + 2, rw = (SDM_PLATE_TW >> j) + 2;
    const int oy = by * (SDM_PLATE_TH >> j) - 1, ox = bx * (SDM_PLATE_TW >> j) - 1;
    const int hj = plate_dim(H, lf + j), wj = plate_dim(W, lf + j);
    const f32x4* pl = j == n ? coarse : j == 1 ? m1 : m2;
    if (j < n) __syncthreads();                                         // the coarser region is complete
    for (int idx = tid; idx < rh * rw; idx += 256) {
      const int ry = idx / rw, rx = idx - ry * rw, y = oy + ry, x = ox + rx;
      if (y < 0 || y >= hj || x < 0 || x >= wj) continue;               // never read: see plate_up
      const f32x4 cw = pl[((size_t)b * hj + y) * wj + x];
      reg[idx] = j == n ? cw : plate_up(nb, rw / 2 + 1, by * (SDM_PLATE_TH >> (j + 1)) - 1, bx * (SDM_PLATE_TW >> (j + 1)) - 1, plate_dim(H, lf + j + 1),
                                        plate_dim(W, lf + j + 1), y, x, cw);
    }
  }
  __syncthreads();
  // the tile itself: 16 runs of 4 pixels per row, 32 rows, two runs per thread
  const int hc = plate_dim(H, lf + 1), wc = plate_dim(W, lf + 1);
  const int coy = by * (SDM_PLATE_TH / 2) - 1, cox = bx * (SDM_PLATE_TW / 2) - 1;
#pragma unroll
  for (int rr = 0; rr < 2; ++rr) {
    const int run = tid + 256 * rr;
    const int y = by * SDM_PLATE_TH + (run >> 4), x = bx * SDM_PLATE_TW + 4 * (run & 15);
    const int npx = y < hf ? max(0, min(4, wf - x)) : 0;
    if (npx == 0) continue;
    const size_t g = ((size_t)b * hf + y) * wf + x;
    f32x4 p[4];
    if (lf == 0) plate_load0(in, g, npx, p);
    else {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (i < npx) p[i] = fine[g + i];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (i < npx) p[i] = plate_up(r1, SDM_PLATE_TW / 2 + 2, coy, cox, hc, wc, y, x + i, p[i]);
    if (lf != 0) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (i < npx) fine[g + i] = p[i];
    } else if (in.vec) {                                                // (npx == 4: W % 4 == 0)
      f32x4* op = (f32x4*)(out + g * 3);
      op[0] = f32x4{p[0][0], p[0][1], p[0][2], p[1][0]};
      op[1] = f32x4{p[1][1], p[1][2], p[2][0], p[2][1]};
      op[2] = f32x4{p[2][2], p[3][0], p[3][1], p[3][2]};
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (i < npx) { float* o = out + (g + i) * 3; o[0] = p[i][0]; o[1] = p[i][1]; o[2] = p[i][2]; }
    }
  }
}
