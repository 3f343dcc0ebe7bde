// k_key.h - green-screen shots: the screen's colour, the colour-difference key, a trimap from the key, despill (sdm_screen_colour and sdm_chroma_key in
// include/sdmatte.h, which is the normative text; DESIGN.md 4, "key").
//
//   screen colour   a pixel is ELIGIBLE iff s = (r + g) + b >= 0.15, max - min >= 0.25 s and the hint's channel is strictly the largest; its BIN is
//                   (iu, iv) = (min(63, (int)(r / s * 64)), min(63, (int)(g / s * 64))) of a 64 x 64 histogram per slot (an image, or the whole batch laid end
//                   to end with share).  The mode is the bin of the largest 3 x 3 sum (lowest index on a tie); the colour is the mean of the eligible
//                   pixels of the mode's 3 x 3 neighbourhood.
//   key             S = the pixel's screen colour, k = its largest channel, y(v) = the larger of the other two, m = c[k] - y(c), mS = S[k] - y(S);
//                   valid iff mS >= 1/64 and m finite; key = clamp01((clip_bg mS - m) / ((clip_bg - clip_fg) mS)), 1 where not valid; class F / B / U by
//                   m <= sure_fg mS / m >= sure_bg mS; despilled[k] = c[k] - despill max(m, 0).
// sdm_screen_colour is FIVE launches, whatever the content:
//   ck_clear_kernel     zeroes the slots' histograms in the arena.
//   ck_hist_kernel      a block owns SDM_KEY_HIST_PX = 16384 consecutive pixels of one slot, a thread 16 groups of 4 pixels (ts_load: 16-byte loads when the
//                       slot's pixel count % 4 == 0 and the image is aligned, scalar loads otherwise, one arithmetic path).  The 4096 int bins sit in 16 KB of
//                       LDS.  A screen puts most lanes into the same few bins and same-address LDS atomics serialise, so equal bins are added together: a
//                       thread adds each run of equal bins among its 4 pixels with one atomicAdd(int); when all 256 pixels of a wave's step fall into ONE bin
//                       (or are all ineligible) no lane adds anything, the wave carries (bin, count) to the next step, and one lane adds the total when the
//                       bin changes.  Only non-zero bins go to the slot's histogram in global memory, with integer atomicAdd: the result does not depend on
//                       the order.
//   ck_mode_kernel      one block per slot: the histogram goes through LDS, a thread forms the 3 x 3 sums of its 16 bins, the argmax (larger sum, then
//                       smaller index: a total order, so any tree gives the same bin) and the eligible count go over the wave by shuffles and over the four
//                       waves in LDS.
//   ck_mean_kernel      one block per run of SDM_KEY_RUN_PX = 4096 pixels of a slot, the summation contract of hz_stats_kernel: a thread sums the selected
//                       ones of its 16 pixels in index order, the wave by a butterfly, the four waves in wave order; the count is an int.  {r, g, b, n}.
//   ck_finalize_kernel  one wave per slot: the runs go through LDS 1024 at a time, lanes 0 .. 3 add one of the four sums each in ascending run order (fp64;
//                       the count in 64-bit integers), thread 0 divides and rounds once, and the wave writes the rows of the slot's images.
// sdm_chroma_key is ONE launch without a trimap and FOUR with one:
//   ck_key_kernel       pointwise, a thread 4 consecutive pixels of the batch (16-byte loads and stores when every tensor given is aligned; the ragged last
//                       group and unaligned tensors take scalar accesses, one arithmetic path): key, class bytes (1 F, 0 B, 2 U; only with a trimap) and
//                       despilled, whichever are asked for.
//   trimap_cols_kernel, trimap_rows_kernel (k_trimap.h, unchanged) on the key at threshold 0.5.
//   ck_veto_kernel      the trimap keeps a definite value only where the pixel's class agrees.
// No load leaves the tensors: a group of 4 pixels is fetched whole only where all 4 exist (the vector path needs npx == 4 or a pixel count % 4 == 0), the
// scalar path touches the npx pixels that exist, a bin index is clamped to [0, 63] before it is used (a negative or NaN quotient goes to bin 0), and the
// partials are indexed by (slot, run) below the counts the host allocated.
#pragma once
#include "sdm_common.h"
#include "k_temporal.h"    // ts_load

#define SDM_KEY_BINS 64                                                 // bins per chromaticity axis
#define SDM_KEY_NBIN (SDM_KEY_BINS * SDM_KEY_BINS)                      // 4096 ints = 16 KB of LDS
#define SDM_KEY_HIST_PX 16384                                           // pixels of a ck_hist_kernel block: 256 threads x 16 groups x 4 pixels
#define SDM_KEY_RUN_PX 4096                                             // SDM_KEY_RUN: pixels of a run = 256 threads x 4 groups x 4 pixels
#define SDM_KEY_FIN_CHUNK 1024                                          // runs in LDS at a time in ck_finalize_kernel (16 KB)
#define SDM_KEY_CLS_F 1                                                 // class bytes
#define SDM_KEY_CLS_B 0
#define SDM_KEY_CLS_U 2

struct CkPartial { float r, g, b; int n; };                             // one run's sums over its selected pixels
struct CkKeyParams { float clip_fg, clip_bg, sure_fg, sure_bg, despill, min_sep; };
struct CkColourParams { float min_sum, min_sat; int hint; };

// the bin iu * 64 + iv of an eligible pixel, -1 otherwise
SDM_DEV_INLINE int ck_bin(float r, float g, float b, CkColourParams prm) {
#pragma clang fp contract(off)
  const float s = (r + g) + b;
  float mx = r, mn = r;
  if (g > mx) mx = g;
  if (b > mx) mx = b;
  if (g < mn) mn = g;
  if (b < mn) mn = b;
  bool ok = s >= prm.min_sum && (mx - mn) >= prm.min_sat * s;
  if (prm.hint == 1) ok = ok && g > r && g > b;
  if (prm.hint == 2) ok = ok && b > r && b > g;
  if (!ok) return -1;
  const float u = (r / s) * 64.0f, v = (g / s) * 64.0f;
  const int iu = u >= 0.0f ? (u < 64.0f ? (int)u : 63) : 0;             // (a NaN fails the first compare)
  const int iv = v >= 0.0f ? (v < 64.0f ? (int)v : 63) : 0;
  return iu * SDM_KEY_BINS + iv;
}

// channel k of (r, g, b) and the larger of the other two (o1 < o2; o2 on a tie or a NaN)
SDM_DEV_INLINE void ck_split(float r, float g, float b, int k, float& top, float& other) {
  if (k == 0) { top = r; other = g > b ? g : b; }
  else if (k == 1) { top = g; other = r > b ? r : b; }
  else { top = b; other = r > g ? r : g; }
}

// grid: ceil(n / 256) blocks of 256 threads
__global__ __launch_bounds__(256) void ck_clear_kernel(int* __restrict__ hist, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) hist[i] = 0;
}

// grid: slots * ceil(P / 16384) blocks of 256 threads.  P: pixels of a slot; vec: P % 4 == 0 and image 16-byte aligned.  hist: [slots][4096].
__global__ __launch_bounds__(256) void ck_hist_kernel(const float* __restrict__ image, int slots, int P, CkColourParams prm, int vec, int* __restrict__ hist) {
  SDM_SHARED int bins[SDM_KEY_NBIN];
  const int tid = threadIdx.x, lane = tid & 63;
  const int nblk = (P + SDM_KEY_HIST_PX - 1) / SDM_KEY_HIST_PX;
  const int slot = blockIdx.x / nblk, blk = blockIdx.x - slot * nblk;
  const size_t base = (size_t)slot * P;
  for (int i = tid; i < SDM_KEY_NBIN; i += 256) bins[i] = 0;
  __syncthreads();
  int wbin = -1, wcnt = 0;                                              // the wave's pending bin and count (the same in every lane)
  for (int it = 0; it < 16; ++it) {
    const int i = blk * SDM_KEY_HIST_PX + (it * 256 + tid) * 4;         // pixel index in the slot: a multiple of 4
    const int npx = max(0, min(4, P - i));
    int bn[4] = {-1, -1, -1, -1};
    if (npx > 0) {
      float c[12], dummy[4];
      ts_load(image, image, base + i, npx, vec != 0, false, c, dummy);
#pragma unroll
      for (int k = 0; k < 4; ++k) if (k < npx) bn[k] = ck_bin(c[3 * k], c[3 * k + 1], c[3 * k + 2], prm);
    }
    const int first = __shfl(bn[0], 0);
    const int one = !__any((int)(bn[0] != first || bn[1] != first || bn[2] != first || bn[3] != first));
    if (one && first == wbin) { wcnt += 256; continue; }                // (wave-uniform from here on)
    if (wcnt > 0 && wbin >= 0 && lane == 0) atomicAdd(&bins[wbin], wcnt);
    wbin = -1; wcnt = 0;
    if (one) { wbin = first; wcnt = 256; continue; }
    int cur = bn[0], cnt = 1;
#pragma unroll
    for (int k = 1; k < 4; ++k) {
      if (bn[k] == cur) { ++cnt; continue; }
      if (cur >= 0) atomicAdd(&bins[cur], cnt);
      cur = bn[k]; cnt = 1;
    }
    if (cur >= 0) atomicAdd(&bins[cur], cnt);
  }
  if (wcnt > 0 && wbin >= 0 && lane == 0) atomicAdd(&bins[wbin], wcnt);
  __syncthreads();
  for (int i = tid; i < SDM_KEY_NBIN; i += 256) {
    const int v = bins[i];
    if (v != 0) atomicAdd(&hist[(size_t)slot * SDM_KEY_NBIN + i], v);
  }
}

// grid: slots blocks of 256 threads.  mode: [slots][2] = {eligible pixels, mode bin or -1}.
__global__ __launch_bounds__(256) void ck_mode_kernel(const int* __restrict__ hist, int* __restrict__ mode) {
  SDM_SHARED int bins[SDM_KEY_NBIN];
  SDM_SHARED int red[4][3];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, slot = blockIdx.x;
  for (int i = tid; i < SDM_KEY_NBIN; i += 256) bins[i] = hist[(size_t)slot * SDM_KEY_NBIN + i];
  __syncthreads();
  int best = -1, bidx = 0, total = 0;
  for (int j = 0; j < 16; ++j) {
    const int idx = tid * 16 + j, iu = idx >> 6, iv = idx & 63;
    int c = 0;
    for (int du = -1; du <= 1; ++du)
      for (int dv = -1; dv <= 1; ++dv) {
        const int u = iu + du, v = iv + dv;
        if (u >= 0 && u < SDM_KEY_BINS && v >= 0 && v < SDM_KEY_BINS) c += bins[u * SDM_KEY_BINS + v];
      }
    total += bins[idx];
    if (c > best) { best = c; bidx = idx; }                             // ascending idx: the first of equal sums stays
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    const int ob = __shfl_xor(best, d), oi = __shfl_xor(bidx, d);
    total += __shfl_xor(total, d);
    if (ob > best || (ob == best && oi < bidx)) { best = ob; bidx = oi; }
  }
  if (lane == 0) { red[wv][0] = best; red[wv][1] = bidx; red[wv][2] = total; }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < 4; ++w) {
      if (red[w][0] > best || (red[w][0] == best && red[w][1] < bidx)) { best = red[w][0]; bidx = red[w][1]; }
      total += red[w][2];
    }
    mode[slot * 2] = total;
    mode[slot * 2 + 1] = total > 0 ? bidx : -1;
  }
}

// grid: slots * ceil(P / 4096) blocks of 256 threads.  partials: [slots][runs].
__global__ __launch_bounds__(256) void ck_mean_kernel(const float* __restrict__ image, int slots, int P, CkColourParams prm, int vec,
                                                      const int* __restrict__ mode, CkPartial* __restrict__ partials) {
#pragma clang fp contract(off)
  SDM_SHARED float red[4][3];
  SDM_SHARED int redn[4];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int runs = (P + SDM_KEY_RUN_PX - 1) / SDM_KEY_RUN_PX;
  const int slot = blockIdx.x / runs, run = blockIdx.x - slot * runs;
  const size_t base = (size_t)slot * P;
  const int mbin = mode[slot * 2 + 1], mu = mbin >> 6, mv = mbin & 63;    // (the same for the whole block)
  float s[3] = {0.0f, 0.0f, 0.0f};
  int n = 0;
  if (mbin >= 0) {
    for (int half = 0; half < 2; ++half) {                              // two groups' loads are in flight together
      float c[2][12];
      int npx[2];
#pragma unroll
      for (int it = 0; it < 2; ++it) {
        const int i = run * SDM_KEY_RUN_PX + ((2 * half + it) * 256 + tid) * 4;
        npx[it] = max(0, min(4, P - i));
        float dummy[4];
        if (npx[it] > 0) ts_load(image, image, base + i, npx[it], vec != 0, false, c[it], dummy);
      }
#pragma unroll
      for (int it = 0; it < 2; ++it) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (k < npx[it]) {
            const int bn = ck_bin(c[it][3 * k], c[it][3 * k + 1], c[it][3 * k + 2], prm);
            const int du = (bn >> 6) - mu, dv = (bn & 63) - mv;
            if (bn >= 0 && du >= -1 && du <= 1 && dv >= -1 && dv <= 1) {
              s[0] += c[it][3 * k]; s[1] += c[it][3 * k + 1]; s[2] += c[it][3 * k + 2];
              n += 1;
            }
          }
        }
      }
    }
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
#pragma unroll
    for (int k = 0; k < 3; ++k) s[k] += __shfl_xor(s[k], d);
    n += __shfl_xor(n, d);
  }
  if (lane == 0) { red[wv][0] = s[0]; red[wv][1] = s[1]; red[wv][2] = s[2]; redn[wv] = n; }
  __syncthreads();
  if (tid == 0) {
    CkPartial p;
    p.r = ((red[0][0] + red[1][0]) + red[2][0]) + red[3][0];
    p.g = ((red[0][1] + red[1][1]) + red[2][1]) + red[3][1];
    p.b = ((red[0][2] + red[1][2]) + red[2][2]) + red[3][2];
    p.n = ((redn[0] + redn[1]) + redn[2]) + redn[3];
    partials[(size_t)slot * runs + run] = p;
  }
}

// grid: slots blocks of 64 threads.  per: images per slot (the slot's images are rows slot * per .. + per - 1 of screen / info).  info: null or [B][4].
__global__ __launch_bounds__(64) void ck_finalize_kernel(const CkPartial* __restrict__ partials, const int* __restrict__ mode, int runs, int per,
                                                         float* __restrict__ screen, int* __restrict__ info) {
  SDM_SHARED float vals[3][SDM_KEY_FIN_CHUNK];                          // one row per sum: a lane's reads are consecutive, so they can be wide and early
  SDM_SHARED int cnt[SDM_KEY_FIN_CHUNK];
  SDM_SHARED double tot[3];
  SDM_SHARED long long totn;
  const int lane = threadIdx.x, slot = blockIdx.x;
  double acc = 0.0;
  long long accn = 0;
  for (int r0 = 0; r0 < runs; r0 += SDM_KEY_FIN_CHUNK) {
    const int nr = min(SDM_KEY_FIN_CHUNK, runs - r0);
    __syncthreads();
    for (int j = lane; j < nr; j += 64) {
      const CkPartial p = partials[(size_t)slot * runs + r0 + j];
      vals[0][j] = p.r; vals[1][j] = p.g; vals[2][j] = p.b; cnt[j] = p.n;
    }
    __syncthreads();
    if (lane < 3) {                                                     // one dependent fp64 add per run: the loads of 8 runs go ahead of their adds
      const float* v = vals[lane];
      int j = 0;
      for (; j + 8 <= nr; j += 8) {
        float t[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) t[k] = v[j + k];
#pragma unroll
        for (int k = 0; k < 8; ++k) acc += (double)t[k];
      }
      for (; j < nr; ++j) acc += (double)v[j];
    } else if (lane == 3) {
      for (int j = 0; j < nr; ++j) accn += cnt[j];
    }
  }
  if (lane < 3) tot[lane] = acc;
  if (lane == 3) totn = accn;
  __syncthreads();
  const int eligible = mode[slot * 2], mbin = mode[slot * 2 + 1];
  const long long n = totn;
  for (int j = lane; j < per * 3; j += 64) screen[(size_t)slot * per * 3 + j] = n > 0 ? (float)(tot[j % 3] / (double)n) : 0.0f;
  if (info) {
    for (int j = lane; j < per * 4; j += 64) {
      const int k = j & 3;
      info[(size_t)slot * per * 4 + j] = k == 0 ? eligible : (k == 1 ? (int)n : (mbin < 0 ? -1 : (k == 2 ? mbin >> 6 : mbin & 63)));
    }
  }
}

// grid: ceil(ceil(B H W / 4) / 256) blocks of 256 threads.  screen: [B][3], or [B][H][W][3] with plane.  key, cls, desp: null = not wanted.  vec: every
// tensor given is 16-byte aligned.
__global__ __launch_bounds__(256) void ck_key_kernel(const float* __restrict__ image, const float* __restrict__ screen, int plane, int B, int HW,
                                                     CkKeyParams prm, int vec, float* __restrict__ key, unsigned char* __restrict__ cls,
                                                     float* __restrict__ desp) {
#pragma clang fp contract(off)
  const long long total = (long long)B * HW;
  const long long g0 = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (g0 >= total) return;
  const int npx = (int)(total - g0 < 4 ? total - g0 : 4);
  const bool wide = vec != 0 && npx == 4;
  float c[12], sp[12], dummy[4];
  ts_load(image, image, (size_t)g0, npx, wide, false, c, dummy);
  if (plane) ts_load(screen, screen, (size_t)g0, npx, wide, false, sp, dummy);
  else {                                                                // a colour per image: every pixel of the group looks its own image up
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int b = (int)((g0 + (i < npx ? i : 0)) / HW);
      sp[3 * i] = screen[b * 3]; sp[3 * i + 1] = screen[b * 3 + 1]; sp[3 * i + 2] = screen[b * 3 + 2];
    }
  }
  float kq[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  unsigned int cq = 0;                                                  // the four class bytes, pixel i in byte i
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (i < npx) {
      const float S[3] = {sp[3 * i], sp[3 * i + 1], sp[3 * i + 2]};
      int k = 0;
      if (S[1] > S[0]) k = 1;
      if (S[2] > (k ? S[1] : S[0])) k = 2;
      float ck, yc, Sk, yS;
      ck_split(c[3 * i], c[3 * i + 1], c[3 * i + 2], k, ck, yc);
      ck_split(S[0], S[1], S[2], k, Sk, yS);
      const float m = ck - yc, mS = Sk - yS;
      const bool valid = mS >= prm.min_sep && fabsf(m) <= 3.402823466e38f;
      float kv = 1.0f;
      unsigned int cv = SDM_KEY_CLS_U;
      if (valid) {
        const float t = prm.clip_bg * mS;
        const float q = (t - m) / ((prm.clip_bg - prm.clip_fg) * mS);
        kv = q > 0.0f ? (q < 1.0f ? q : 1.0f) : 0.0f;
        if (m <= prm.sure_fg * mS) cv = SDM_KEY_CLS_F;
        else if (m >= prm.sure_bg * mS) cv = SDM_KEY_CLS_B;
        // c becomes the despilled pixel; the other channels stay bit copies (selects with constant indices: a store under `k == ...` would become a
        // store at a variable index and send the array to scratch memory)
        const float d = ck - prm.despill * m;
        const bool spill = m > 0.0f;
        c[3 * i] = spill && k == 0 ? d : c[3 * i];
        c[3 * i + 1] = spill && k == 1 ? d : c[3 * i + 1];
        c[3 * i + 2] = spill && k == 2 ? d : c[3 * i + 2];
      }
      kq[i] = kv; cq |= cv << (8 * i);
    }
  }
  if (wide) {
    if (key) { f32x4 v; v[0] = kq[0]; v[1] = kq[1]; v[2] = kq[2]; v[3] = kq[3]; *(f32x4*)(key + g0) = v; }
    if (desp) {
      f32x4* dp = (f32x4*)(desp + g0 * 3);
#pragma unroll
      for (int j = 0; j < 3; ++j) { f32x4 v; v[0] = c[4 * j]; v[1] = c[4 * j + 1]; v[2] = c[4 * j + 2]; v[3] = c[4 * j + 3]; dp[j] = v; }
    }
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (i < npx) {
        if (key) key[g0 + i] = kq[i];
        if (desp) { desp[(g0 + i) * 3] = c[3 * i]; desp[(g0 + i) * 3 + 1] = c[3 * i + 1]; desp[(g0 + i) * 3 + 2] = c[3 * i + 2]; }
      }
    }
  }
  if (cls) {                                                            // (the plane lives in the arena: g0 is a multiple of 4, so the word is aligned)
    if (npx == 4) *(unsigned int*)(cls + g0) = cq;
    else {
#pragma unroll
      for (int i = 0; i < 3; ++i) if (i < npx) cls[g0 + i] = (unsigned char)(cq >> (8 * i));
    }
  }
}

// grid: ceil(n / 256) blocks of 256 threads.  In place: trimap holds T0 and gets T.
__global__ __launch_bounds__(256) void ck_veto_kernel(float* __restrict__ trimap, const unsigned char* __restrict__ cls, long long n) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float t0 = trimap[i];
  const int c = cls[i];
  const bool keep = (t0 == 1.0f && c == SDM_KEY_CLS_F) || (t0 == 0.0f && c == SDM_KEY_CLS_B) || t0 == 0.5f;
  if (!keep) trimap[i] = 0.5f;
}
