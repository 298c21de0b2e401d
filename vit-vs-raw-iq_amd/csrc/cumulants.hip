// Cumulant classifier (iq_frames_cumulants, include/iqvit.h): the mean, the ten central moments up to order eight and the ten
// cumulant features of every frame, the distance of the features to every class's centroid, and the decision -- one launch.
// The definition, with every rounding, is in the header.
//
// Two passes over a frame that is read from memory once.  Pass one loads each sample, adds it to the lane's sum for the mean and
// puts it into LDS in the slot of its own index; pass two reads the slots back, subtracts the mean and adds the 17 powers
// (symbol_terms).  A thread reads only the slots it wrote itself, so the frame in LDS needs no barrier: LDS is a register file
// that a run-time length can index.  Two routes, by the length alone:
//   len <= CUM_WAVE_LEN (256)   one WAVE per frame, FR_WAVES frames per workgroup: lane l takes the symbols l, l + 64, ...; the
//                               butterfly leaves every sum in every lane; no barrier at all, a wave without a frame leaves
//   len >  CUM_WAVE_LEN         one WORKGROUP per frame: thread t takes t, t + 256, ...; the butterfly, then the four wave sums
//                               through LDS in ascending order (red_sum); wave 0 goes on alone
// (a batch of 128-symbol frames on the second route would run three waves of four on nothing, and launch four times the
// workgroups).  Then every lane of the frame's wave does the cumulant algebra on the same numbers (one lane's work, 64 times over:
// nothing to broadcast), lane c < C forms score[c] against its class's row, and lane 0 walks the scores c ascending through
// shuffles.  No atomics, no workspace; the order of every sum is fixed by (len, the route), so two runs agree bit for bit and a
// frame's outputs depend on neither n_frames nor its position.
//
// Indices.  LDS: slot n < len of the frame's part, keep + wave * len on the wave route ((FR_WAVES - 1) * len + n < FR_WAVES * len,
// the size asked for), keep on the workgroup route (n < len); red[(2 + 17) * FR_WAVES] static.  Memory: frame fi < n_frames at
// x + fi 2 len (long), sample n < len; mom at fi 20 + k, feat at fi 10 + f, score at fi C + c with c < C, pred and sigma2 at fi; mu
// and w at c 10 + f, bias at c, c < C.
#include <math.h>

#include "frames.h"
#include "iqvit.h"
#include "prof.h"

#pragma clang fp contract(off)       // a product and a sum are fused where fmaf says so and nowhere else

namespace {

constexpr int CUM_FEATS = 10, CUM_MOMS = 20, CUM_SUMS = 17, CUM_MAX_CLASSES = 64;
constexpr int CUM_WAVE_LEN = 256;    // the longest frame of the wave-per-frame route: four symbols per lane

struct CumArgs {
  const float* x;
  const float* sigma2;
  const float* mu;
  const float* w;
  const float* bias;
  float* feat;
  float* mom;
  float* score;
  int* pred;
  int n_frames, len, n_classes, planar;
};

// complex arithmetic on (re, im), every rounding spelled out
__device__ __forceinline__ float2 cmul(float2 a, float2 b) {
  return make_float2(fmaf(a.x, b.x, -__fmul_rn(a.y, b.y)), fmaf(a.x, b.y, __fmul_rn(a.y, b.x)));
}
__device__ __forceinline__ float2 cmulc(float2 a, float2 b) {      // conj(a) b
  return make_float2(fmaf(a.x, b.x, __fmul_rn(a.y, b.y)), fmaf(a.x, b.y, -__fmul_rn(a.y, b.x)));
}
__device__ __forceinline__ float2 csq(float2 a) {
  return make_float2(fmaf(a.x, a.x, -__fmul_rn(a.y, a.y)), __fmul_rn(__fadd_rn(a.x, a.x), a.y));
}
__device__ __forceinline__ float norm2(float2 a) { return fmaf(a.y, a.y, __fmul_rn(a.x, a.x)); }
__device__ __forceinline__ float cabs_rn(float2 a) { return sqrtf(norm2(a)); }
__device__ __forceinline__ float2 caxpy(float s, float2 a, float2 b) { return make_float2(fmaf(s, a.x, b.x), fmaf(s, a.y, b.y)); }

// The 17 terms of one centred symbol z = (a, b), in mom's order behind the mean: z^2, |z|^2, z^4, z^2 |z|^2, |z|^4, z^6,
// z^4 |z|^2, z^2 |z|^4, |z|^6, z^8
__device__ __forceinline__ void symbol_terms(float a, float b, float* t) {
  const float2 z2 = csq(make_float2(a, b)), z4 = csq(z2), z6 = cmul(z4, z2), z8 = csq(z4);
  const float r = norm2(make_float2(a, b)), r2 = __fmul_rn(r, r);
  t[0] = z2.x; t[1] = z2.y; t[2] = r;
  t[3] = z4.x; t[4] = z4.y; t[5] = __fmul_rn(z2.x, r); t[6] = __fmul_rn(z2.y, r); t[7] = r2;
  t[8] = z6.x; t[9] = z6.y; t[10] = __fmul_rn(z4.x, r); t[11] = __fmul_rn(z4.y, r);
  t[12] = __fmul_rn(z2.x, r2); t[13] = __fmul_rn(z2.y, r2); t[14] = __fmul_rn(r2, r);
  t[15] = z8.x; t[16] = z8.y;
}

template <bool GROUP>
__global__ __launch_bounds__(FR_THREADS) void frames_cumulants_kernel(CumArgs a) {
  extern __shared__ float2 keep[];
  __shared__ float red[(2 + CUM_SUMS) * FR_WAVES];
  const int tid = threadIdx.x, lane = tid & (IQ_WAVE - 1), wave = tid >> 6;
  const int len = a.len, C = a.n_classes;
  const long fi = GROUP ? (long)blockIdx.x : (long)blockIdx.x * FR_WAVES + wave;
  if (!GROUP && fi >= a.n_frames) return;                  // (the wave route holds no barrier)
  const int first = GROUP ? tid : lane, stride = GROUP ? FR_THREADS : IQ_WAVE;
  float2* mine = keep + (GROUP ? 0 : wave * len);
  const float* src = a.x + fi * 2 * len;

  // pass one: the mean
  float sr = 0.f, si = 0.f;
  for (int n = first; n < len; n += stride) {
    const float2 v = load_sample(src, len, a.planar, n);
    mine[n] = v;
    sr = __fadd_rn(sr, v.x);
    si = __fadd_rn(si, v.y);
  }
  sr = wave_sum(sr);
  si = wave_sum(si);
  if (GROUP) {
    if (lane == 0) { red[wave] = sr; red[FR_WAVES + wave] = si; }
    __syncthreads();
    sr = red_sum(red);
    si = red_sum(red + FR_WAVES);
  }
  const float flen = (float)len;
  const float mr = __fdiv_rn(sr, flen), mi = __fdiv_rn(si, flen);

  // pass two: the 17 central sums
  float s[CUM_SUMS];
#pragma unroll
  for (int k = 0; k < CUM_SUMS; ++k) s[k] = 0.f;
  for (int n = first; n < len; n += stride) {
    const float2 v = mine[n];
    float t[CUM_SUMS];
    symbol_terms(__fsub_rn(v.x, mr), __fsub_rn(v.y, mi), t);
#pragma unroll
    for (int k = 0; k < CUM_SUMS; ++k) s[k] = __fadd_rn(s[k], t[k]);
  }
#pragma unroll
  for (int k = 0; k < CUM_SUMS; ++k) s[k] = wave_sum(s[k]);
  if (GROUP) {
    float* r2 = red + 2 * FR_WAVES;
    if (lane == 0) {
#pragma unroll
      for (int k = 0; k < CUM_SUMS; ++k) r2[k * FR_WAVES + wave] = s[k];
    }
    __syncthreads();
    if (wave != 0) return;                                 // (behind the last barrier)
#pragma unroll
    for (int k = 0; k < CUM_SUMS; ++k) s[k] = red_sum(r2 + k * FR_WAVES);
  }
#pragma unroll
  for (int k = 0; k < CUM_SUMS; ++k) s[k] = __fdiv_rn(s[k], flen);

  // the algebra of the header, on the same numbers in every lane
  const float2 M20 = make_float2(s[0], s[1]), M40 = make_float2(s[3], s[4]), M41 = make_float2(s[5], s[6]);
  const float2 M60 = make_float2(s[8], s[9]), M61 = make_float2(s[10], s[11]), M62 = make_float2(s[12], s[13]);
  const float2 M80 = make_float2(s[15], s[16]);
  const float M21 = s[2], M42 = s[7], M63 = s[14];
  const float2 q = csq(M20);                               // M20^2
  const float n20 = norm2(M20);                            // |M20|^2
  const float2 C40 = caxpy(-3.f, q, M40);
  const float2 C41 = caxpy(-__fmul_rn(3.f, M21), M20, M41);
  const float C42 = fmaf(-__fadd_rn(M21, M21), M21, __fsub_rn(M42, n20));
  const float2 C60 = caxpy(30.f, cmul(q, M20), caxpy(-15.f, cmul(M20, M40), M60));
  const float2 C61 = caxpy(__fmul_rn(30.f, M21), q, caxpy(-10.f, cmul(M20, M41), caxpy(-__fmul_rn(5.f, M21), M40, M61)));
  const float2 e62 = caxpy(-__fmul_rn(8.f, M21), M41, caxpy(-__fmul_rn(6.f, M42), M20, M62));
  const float2 v62 = cmulc(M20, M40);
  const float g62 = fmaf(__fmul_rn(24.f, M21), M21, __fmul_rn(6.f, n20));
  const float2 C62 = caxpy(g62, M20, make_float2(__fsub_rn(e62.x, v62.x), __fsub_rn(e62.y, v62.y)));
  const float h63 = fmaf(M20.x, M41.x, __fmul_rn(M20.y, M41.y));                  // Re(M20 conj M41) = Re(conj(M20) M41)
  const float C63 = fmaf(__fmul_rn(18.f, n20), M21,
                         fmaf(-6.f, h63, fmaf(__fmul_rn(12.f, __fmul_rn(M21, M21)), M21, fmaf(-__fmul_rn(9.f, M21), M42, M63))));
  const float2 C80 = caxpy(-630.f, csq(q), caxpy(420.f, cmul(q, M40), caxpy(-35.f, csq(M40), caxpy(-28.f, cmul(M20, M60), M80))));
  const float P = __fsub_rn(M21, a.sigma2 ? a.sigma2[fi] : 0.f);
  const bool ok = P > 0.f && P < INFINITY;                 // P is data: a frame without a signal variance gets NaN
  const float P2 = __fmul_rn(P, P), P3 = __fmul_rn(P2, P), P4 = __fmul_rn(P3, P);
  const float nan = nanf("");
  float f[CUM_FEATS];
  f[0] = __fdiv_rn(norm2(make_float2(mr, mi)), P);
  f[1] = __fdiv_rn(cabs_rn(M20), P);
  f[2] = __fdiv_rn(cabs_rn(C40), P2);
  f[3] = __fdiv_rn(cabs_rn(C41), P2);
  f[4] = __fdiv_rn(C42, P2);
  f[5] = __fdiv_rn(cabs_rn(C60), P3);
  f[6] = __fdiv_rn(cabs_rn(C61), P3);
  f[7] = __fdiv_rn(cabs_rn(C62), P3);
  f[8] = __fdiv_rn(C63, P3);
  f[9] = __fdiv_rn(cabs_rn(C80), P4);
#pragma unroll
  for (int k = 0; k < CUM_FEATS; ++k) f[k] = ok ? f[k] : nan;

  if (lane == 0) {
    if (a.mom) {
      float* o = a.mom + fi * CUM_MOMS;
      o[0] = mr; o[1] = mi;
#pragma unroll
      for (int k = 0; k < CUM_SUMS; ++k) o[2 + k] = s[k];
      o[2 + CUM_SUMS] = P;
    }
    if (a.feat) {
      float* o = a.feat + fi * CUM_FEATS;
#pragma unroll
      for (int k = 0; k < CUM_FEATS; ++k) o[k] = f[k];
    }
  }
  if (C == 0) return;

  // lane c < C: the score of class c; then lane 0 walks them
  float sc = nan;
  if (lane < C) {
    const float* mu = a.mu + lane * CUM_FEATS;
    const float* w = a.w + lane * CUM_FEATS;
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < CUM_FEATS; ++k) {
      const float d = __fsub_rn(f[k], mu[k]);
      acc = fmaf(__fmul_rn(w[k], d), d, acc);
    }
    sc = __fsub_rn(a.bias ? a.bias[lane] : 0.f, acc);
    if (a.score) a.score[fi * C + lane] = sc;
  }
  if (a.pred) {
    float best = __shfl(sc, 0, IQ_WAVE);
    int at = 0;
    for (int c = 1; c < C; ++c) {                          // the first largest; a NaN is never larger (nor ever beaten)
      const float v = __shfl(sc, c, IQ_WAVE);
      if (v > best) { best = v; at = c; }
    }
    if (lane == 0) a.pred[fi] = ok ? at : -1;
  }
}

// -> IQ_OK or the refusal; nothing is launched and no device pointer dereferenced before this returns IQ_OK
int check(const float* x, const float* feat, const float* mom, const float* score, const int* pred, int len, const iq_cumulants_t* p) {
  if (!x || !p || (!feat && !mom && !score && !pred)) return IQ_ERR_ARG;
  if (len < 1 || (p->planar & ~1) || p->n_classes < 0) return IQ_ERR_ARG;
  if (p->n_classes > 0 && (!p->mu || !p->w)) return IQ_ERR_ARG;
  if (p->n_classes == 0 && (score || pred)) return IQ_ERR_ARG;
  if ((uintptr_t)x & (p->planar ? 3 : 7)) return IQ_ERR_ARG;         // interleaved frames move as (I, Q) pairs
  if (((uintptr_t)feat | (uintptr_t)mom | (uintptr_t)score | (uintptr_t)pred | (uintptr_t)p->sigma2 | (uintptr_t)p->mu |
       (uintptr_t)p->w | (uintptr_t)p->bias) & 3)
    return IQ_ERR_ARG;
  if (p->n_classes > CUM_MAX_CLASSES || !frame_fits(len)) return IQ_ERR_UNSUPPORTED;
  return IQ_OK;
}

}  // namespace

extern "C" int iq_frames_cumulants(const float* x, float* feat, float* mom, float* score, int* pred, int n_frames, int len,
                                   const iq_cumulants_t* par, iq_stream_t stream) {
  const int rc = check(x, feat, mom, score, pred, len, par);
  if (rc != IQ_OK) return rc;
  if (n_frames <= 0) return IQ_OK;
  const int C = par->n_classes;
  if ((long)n_frames * (C > CUM_MOMS ? C : CUM_MOMS) > INT32_MAX) return IQ_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  CumArgs a = {};
  a.x = x; a.sigma2 = par->sigma2; a.mu = par->mu; a.w = par->w; a.bias = par->bias;
  a.feat = feat; a.mom = mom; a.score = score; a.pred = pred;
  a.n_frames = n_frames; a.len = len; a.n_classes = C; a.planar = par->planar;
  IQ_PROF(IQ_FAM_MISC, st);
  const double bytes = (double)n_frames * (len * 8.0 + (mom ? 80.0 : 0.0) + (feat ? 40.0 : 0.0) + (score ? C * 4.0 : 0.0));
  const double flops = (double)n_frames * (len * 62.0 + C * 40.0);   // 2 + 43 + 17 per symbol: the mean, the terms, the sums
  if (len <= CUM_WAVE_LEN) {
    IQ_PROF_K(bytes, flops, "frames_cumulants_kernel<false>");
    launch_frames(frames_cumulants_kernel<false>, dim3((unsigned)((n_frames + FR_WAVES - 1) / FR_WAVES)),
                  (size_t)FR_WAVES * len * sizeof(float2), st, a);
  } else {
    IQ_PROF_K(bytes, flops, "frames_cumulants_kernel<true>");
    launch_frames(frames_cumulants_kernel<true>, dim3((unsigned)n_frames), (size_t)len * sizeof(float2), st, a);
  }
  return iq_launch_status();
}
