// What the cumulant classifier's forward (cumulants.hip) and backward (cumulants_bwd.hip) share: the complex helpers, the 17 terms
// of a centred symbol, the two passes over a frame in LDS and the cumulant algebra of include/iqvit.h.  The backward recomputes
// the forward's moments and features from the frame; it gets the forward's numbers bit for bit because both run these lines.
#pragma once
#include <math.h>

#include "frames.h"

#pragma clang fp contract(off)       // a product and a sum are fused where fmaf says so and nowhere else

constexpr int CUM_FEATS = 10, CUM_MOMS = 20, CUM_SUMS = 17, CUM_MAX_CLASSES = 64;

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

// floats of static LDS the two passes use: the four wave sums of the mean's two parts and of the 17 terms
constexpr int CUM_RED = (2 + CUM_SUMS) * FR_WAVES;

// Pass one: the frame from memory into LDS, each sample in the slot of its own index, and the mean.  GROUP: one barrier.
template <bool GROUP>
__device__ __forceinline__ float2 cum_mean(const float* src, int len, int planar, float2* mine, float* red, int first, int stride,
                                           int lane, int wave) {
  float sr = 0.f, si = 0.f;
  for (int n = first; n < len; n += stride) {
    const float2 v = load_sample(src, len, planar, n);
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
  return make_float2(__fdiv_rn(sr, flen), __fdiv_rn(si, flen));
}

// Pass two, first half: the 17 central sums of this thread's slots, through the butterfly and, GROUP, into LDS behind one barrier
// (a kernel whose other waves have nothing left to do lets them leave between the halves).
template <bool GROUP>
__device__ __forceinline__ void cum_sums(const float2* mine, int len, float2 m, float* red, int first, int stride, int lane,
                                         int wave, float* s) {
#pragma unroll
  for (int k = 0; k < CUM_SUMS; ++k) s[k] = 0.f;
  for (int n = first; n < len; n += stride) {
    const float2 v = mine[n];
    float t[CUM_SUMS];
    symbol_terms(__fsub_rn(v.x, m.x), __fsub_rn(v.y, m.y), t);
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
  }
}
// Second half: the four waves' sums in ascending order, and the moments
template <bool GROUP>
__device__ __forceinline__ void cum_moments(const float* red, int len, float* s) {
  if (GROUP) {
    const float* r2 = red + 2 * FR_WAVES;
#pragma unroll
    for (int k = 0; k < CUM_SUMS; ++k) s[k] = red_sum(r2 + k * FR_WAVES);
  }
  const float flen = (float)len;
#pragma unroll
  for (int k = 0; k < CUM_SUMS; ++k) s[k] = __fdiv_rn(s[k], flen);
}

// The algebra of the header on the moments s: the cumulants, P and its powers, the ten features (NaN where P is refused)
struct CumAlgebra {
  float2 M20, M40, M41, M60, M61, M62, M80, q, C40, C41, C60, C61, C62, C80;
  float M21, M42, M63, n20, C42, C63, P, P2, P3, P4;
  float f[CUM_FEATS];
  bool ok;
};
__device__ __forceinline__ CumAlgebra cum_algebra(float2 m, const float* s, float sigma2) {
  CumAlgebra c;
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
  const float P = __fsub_rn(M21, sigma2);
  c.ok = P > 0.f && P < INFINITY;                          // P is data: a frame without a signal variance gets NaN
  const float P2 = __fmul_rn(P, P), P3 = __fmul_rn(P2, P), P4 = __fmul_rn(P3, P);
  const float nan = nanf("");
  c.f[0] = __fdiv_rn(norm2(m), P);
  c.f[1] = __fdiv_rn(cabs_rn(M20), P);
  c.f[2] = __fdiv_rn(cabs_rn(C40), P2);
  c.f[3] = __fdiv_rn(cabs_rn(C41), P2);
  c.f[4] = __fdiv_rn(C42, P2);
  c.f[5] = __fdiv_rn(cabs_rn(C60), P3);
  c.f[6] = __fdiv_rn(cabs_rn(C61), P3);
  c.f[7] = __fdiv_rn(cabs_rn(C62), P3);
  c.f[8] = __fdiv_rn(C63, P3);
  c.f[9] = __fdiv_rn(cabs_rn(C80), P4);
#pragma unroll
  for (int k = 0; k < CUM_FEATS; ++k) c.f[k] = c.ok ? c.f[k] : nan;
  c.M20 = M20; c.M40 = M40; c.M41 = M41; c.M60 = M60; c.M61 = M61; c.M62 = M62; c.M80 = M80; c.q = q;
  c.C40 = C40; c.C41 = C41; c.C60 = C60; c.C61 = C61; c.C62 = C62; c.C80 = C80;
  c.M21 = M21; c.M42 = M42; c.M63 = M63; c.n20 = n20; c.C42 = C42; c.C63 = C63;
  c.P = P; c.P2 = P2; c.P3 = P3; c.P4 = P4;
  return c;
}
