// Gradient of the cumulant classifier with respect to the frame (iq_frames_cumulants_bwd, include/iqvit.h): dx = d(sum_c dscore
// score + sum_f dfeat feat) / d(Re y_n, Im y_n), the true gradient, through the mean and through P.  The definition, with every
// rounding, is in the header.
//
// Self-contained: the mean, the 17 central sums and the algebra are recomputed from the frame by the forward's own lines
// (cumulants_common.h), so no forward output is read and nothing is held between the two calls.  The forward's two routes, by the
// length alone (len <= 256: one wave per frame, four frames per workgroup, no barrier; longer: one workgroup per frame).  The
// frame is read from memory once into LDS, a sample in the slot of its own index.  Then
//   pass 1, 2   the mean and the 17 sums, as the forward
//   algebra     in every lane on the same numbers: the class loop (scores -> features; a class whose dscore is 0 is skipped before
//               anything of it is read), features -> cumulants and P, cumulants -> the ten moments, and the thirteen coefficients
//               of the polynomial g(z, conj z) of degree seven; nothing below depends on C
//   pass 3      each thread forms g_n for its own symbols, overwrites its own slot with it and adds it to two running sums
//   the sums    the butterfly and, on the workgroup route, the four waves in ascending order through LDS (one more barrier)
//   pass 4      dx_n = g_n + (gm / len - mean(g)) through store_sample
// A thread touches only slots it wrote itself, so the frame in LDS needs no barrier.  No atomics, no workspace; the order of every
// sum is fixed by (len, the route): two runs agree bit for bit and a frame's dx depends on neither n_frames nor its position.
//
// Indices.  LDS: slot n < len of the frame's part, keep + wave * len on the wave route ((FR_WAVES - 1) * len + n < FR_WAVES * len,
// the size asked for), keep on the workgroup route; red[(2 + 17 + 2) * FR_WAVES] static.  Memory: frame fi < n_frames at x + fi 2 len
// and dx + fi 2 len (long), sample n < len; dscore at fi C + c, c < C; dfeat at fi 10 + f; sigma2 at fi; mu and w at c 10 + f, c < C.
#include <math.h>

#include "cumulants_common.h"
#include "frames.h"
#include "iqvit.h"
#include "prof.h"

#pragma clang fp contract(off)       // a product and a sum are fused where fmaf says so and nowhere else

namespace {

constexpr int CUM_WAVE_LEN = 256;    // the forward's threshold (cumulants.hip): the same two routes at the same lengths

struct CumBwdArgs {
  const float* x;
  const float* dscore;
  const float* dfeat;
  const float* sigma2;
  const float* mu;
  const float* w;
  float* dx;
  int n_frames, len, n_classes, planar;
};

__device__ __forceinline__ float2 cadd(float2 a, float2 b) { return make_float2(__fadd_rn(a.x, b.x), __fadd_rn(a.y, b.y)); }
__device__ __forceinline__ float2 cscale(float s, float2 a) { return make_float2(__fmul_rn(s, a.x), __fmul_rn(s, a.y)); }
__device__ __forceinline__ float2 cdivr(float2 a, float s) { return make_float2(__fdiv_rn(a.x, s), __fdiv_rn(a.y, s)); }
__device__ __forceinline__ float2 conj2(float2 a) { return make_float2(a.x, -a.y); }
__device__ __forceinline__ float dotre(float2 a, float2 b) { return fmaf(a.x, b.x, __fmul_rn(a.y, b.y)); }   // Re(conj(a) b)
// d(|C| / Pk) / dC times gf: gf C / (|C| Pk), and 0 where |C| is 0 (the subgradient)
__device__ __forceinline__ float2 mag_grad(float gf, float2 c, float pk) {
  const float a = cabs_rn(c);
  const float s = __fdiv_rn(gf, __fmul_rn(a, pk));
  return a == 0.f ? make_float2(0.f, 0.f) : cscale(s, c);
}

// the coefficients of g_n = conj(z) k1 + z kz + conj(z^3) k3 + z^3 k3b + conj(z^5) A60 + z^5 B61 + conj(z^7) A80,
// k1 = A20 + r A41 + r^2 A62, kz = A21 + r A42 + r^2 A63, k3 = A40 + r A61, k3b = B41 + r B62
struct CumPoly {
  float2 A20, A41, A62, A40, A61, B41, B62, A60, B61, A80;
  float A21, A42, A63;
};

__device__ __forceinline__ float2 poly_g(const CumPoly& p, float2 z) {
  const float2 z2 = csq(z), z4 = csq(z2);
  const float r = norm2(z), r2 = __fmul_rn(r, r);
  const float2 z3 = cmul(z2, z), z5 = cmul(z4, z), z7 = cmul(z4, z3);
  const float2 k1 = caxpy(r2, p.A62, caxpy(r, p.A41, p.A20));
  const float kz = fmaf(r2, p.A63, fmaf(r, p.A42, p.A21));
  const float2 k3 = caxpy(r, p.A61, p.A40);
  const float2 k3b = caxpy(r, p.B62, p.B41);
  float2 g = cmulc(z, k1);
  g = caxpy(kz, z, g);
  g = cadd(g, cmulc(z3, k3));
  g = cadd(g, cmul(z3, k3b));
  g = cadd(g, cmulc(z5, p.A60));
  g = cadd(g, cmul(z5, p.B61));
  g = cadd(g, cmulc(z7, p.A80));
  return g;
}

template <bool GROUP>
__global__ __launch_bounds__(FR_THREADS) void frames_cumulants_bwd_kernel(CumBwdArgs a) {
  extern __shared__ float2 keep[];
  __shared__ float red[CUM_RED + 2 * FR_WAVES];
  const int tid = threadIdx.x, lane = tid & (IQ_WAVE - 1), wave = tid >> 6;
  const int len = a.len, C = a.n_classes;
  const long fi = GROUP ? (long)blockIdx.x : (long)blockIdx.x * FR_WAVES + wave;
  if (!GROUP && fi >= a.n_frames) return;                  // (the wave route holds no barrier)
  const int first = GROUP ? tid : lane, stride = GROUP ? FR_THREADS : IQ_WAVE;
  float2* mine = keep + (GROUP ? 0 : wave * len);
  const float* src = a.x + fi * 2 * len;
  float* dst = a.dx + fi * 2 * len;

  // passes one and two: the forward's, by the forward's lines
  const float2 m = cum_mean<GROUP>(src, len, a.planar, mine, red, first, stride, lane, wave);
  float s[CUM_SUMS];
  cum_sums<GROUP>(mine, len, m, red, first, stride, lane, wave, s);
  cum_moments<GROUP>(red, len, s);
  const CumAlgebra al = cum_algebra(m, s, a.sigma2 ? a.sigma2[fi] : 0.f);
  const float flen = (float)len;

  // class scores -> features (the only place C shows)
  float gf[CUM_FEATS];
#pragma unroll
  for (int k = 0; k < CUM_FEATS; ++k) gf[k] = a.dfeat ? a.dfeat[fi * CUM_FEATS + k] : 0.f;
  if (a.dscore) {
    for (int c = 0; c < C; ++c) {
      const float ds = a.dscore[fi * C + c];
      if (ds == 0.f) continue;                             // nobody asked about this class: not even its NaNs are read
      const float m2 = __fmul_rn(-2.f, ds);
      const float* mu = a.mu + c * CUM_FEATS;
      const float* w = a.w + c * CUM_FEATS;
#pragma unroll
      for (int k = 0; k < CUM_FEATS; ++k) gf[k] = fmaf(__fmul_rn(m2, w[k]), __fsub_rn(al.f[k], mu[k]), gf[k]);
    }
  }

  // features -> cumulants, P and the mean
  const float2 M20 = al.M20, M40 = al.M40, M41 = al.M41, M60 = al.M60, q = al.q;
  const float M21 = al.M21, M42 = al.M42, n20 = al.n20;
  const float order[CUM_FEATS] = {1.f, 1.f, 2.f, 2.f, 2.f, 3.f, 3.f, 3.f, 3.f, 4.f};
  float accP = 0.f;
#pragma unroll
  for (int k = 0; k < CUM_FEATS; ++k) accP = fmaf(__fmul_rn(order[k], al.f[k]), gf[k], accP);
  const float gP = -__fdiv_rn(accP, al.P);
  const float2 gm = cscale(__fdiv_rn(__fadd_rn(gf[0], gf[0]), al.P), m);
  const float2 gC20 = mag_grad(gf[1], M20, al.P), gC40 = mag_grad(gf[2], al.C40, al.P2), gC41 = mag_grad(gf[3], al.C41, al.P2);
  const float gC42 = __fdiv_rn(gf[4], al.P2);
  const float2 gC60 = mag_grad(gf[5], al.C60, al.P3), gC61 = mag_grad(gf[6], al.C61, al.P3), gC62 = mag_grad(gf[7], al.C62, al.P3);
  const float gC63 = __fdiv_rn(gf[8], al.P3);
  const float2 gC80 = mag_grad(gf[9], al.C80, al.P4);

  // cumulants -> the ten moments: G = dL/dRe M + j dL/dIm M
  const float2 G60 = caxpy(-28.f, cmulc(M20, gC80), gC60);
  float G42 = fmaf(-6.f, dotre(gC62, M20), gC42);
  G42 = fmaf(-__fmul_rn(9.f, M21), gC63, G42);
  float2 G41 = caxpy(-10.f, cmulc(M20, gC61), gC41);
  G41 = caxpy(-__fmul_rn(8.f, M21), gC62, G41);
  G41 = caxpy(__fmul_rn(-6.f, gC63), M20, G41);
  float2 G40 = caxpy(-15.f, cmulc(M20, gC60), gC40);
  G40 = caxpy(-__fmul_rn(5.f, M21), gC61, G40);
  G40 = caxpy(-1.f, cmul(M20, gC62), G40);
  G40 = cadd(G40, cmulc(caxpy(420.f, q, cscale(-70.f, M40)), gC80));
  float G21 = fmaf(-3.f, dotre(gC41, M20), gP);
  G21 = fmaf(-__fmul_rn(4.f, M21), gC42, G21);
  G21 = __fadd_rn(G21, dotre(gC61, caxpy(30.f, q, cscale(-5.f, M40))));
  G21 = __fadd_rn(G21, dotre(gC62, caxpy(__fmul_rn(48.f, M21), M20, cscale(-8.f, M41))));
  G21 = fmaf(gC63, fmaf(18.f, n20, fmaf(__fmul_rn(36.f, M21), M21, __fmul_rn(-9.f, M42))), G21);
  float2 G20 = caxpy(-6.f, cmulc(M20, gC40), gC20);
  G20 = caxpy(-__fmul_rn(3.f, M21), gC41, G20);
  G20 = caxpy(-__fadd_rn(gC42, gC42), M20, G20);
  G20 = cadd(G20, cmulc(caxpy(90.f, q, cscale(-15.f, M40)), gC60));
  G20 = cadd(G20, cmulc(caxpy(__fmul_rn(60.f, M21), M20, cscale(-10.f, M41)), gC61));
  G20 = caxpy(fmaf(__fmul_rn(24.f, M21), M21, fmaf(12.f, n20, __fmul_rn(-6.f, M42))), gC62, G20);
  G20 = cadd(G20, cmulc(gC62, caxpy(6.f, q, make_float2(-M40.x, -M40.y))));
  G20 = caxpy(gC63, caxpy(__fmul_rn(36.f, M21), M20, cscale(-6.f, M41)), G20);
  G20 = cadd(G20, cmulc(caxpy(-2520.f, cmul(q, M20), caxpy(840.f, cmul(M20, M40), cscale(-28.f, M60))), gC80));

  // moments -> the polynomial's coefficients, the same for every symbol of the frame (G61, G62, G63, G80 are gC61, gC62, gC63,
  // gC80: no other cumulant holds those moments)
  CumPoly p;
  p.A20 = cscale(2.f, cdivr(G20, flen));
  p.A21 = __fmul_rn(2.f, __fdiv_rn(G21, flen));
  p.A40 = cscale(4.f, cdivr(G40, flen));
  const float2 H41 = cdivr(G41, flen), H62 = cdivr(gC62, flen), H61 = cdivr(gC61, flen);
  p.A41 = cscale(3.f, H41);
  p.B41 = conj2(H41);
  p.A42 = __fmul_rn(4.f, __fdiv_rn(G42, flen));
  p.A60 = cscale(6.f, cdivr(G60, flen));
  p.A61 = cscale(5.f, H61);
  p.B61 = conj2(H61);
  p.A62 = cscale(4.f, H62);
  p.B62 = conj2(cscale(2.f, H62));
  p.A63 = __fmul_rn(6.f, __fdiv_rn(gC63, flen));
  p.A80 = cscale(8.f, cdivr(gC80, flen));

  // pass three: g_n into the symbol's own slot, and its sum
  float gr = 0.f, gi = 0.f;
  for (int n = first; n < len; n += stride) {
    const float2 v = mine[n];
    const float2 g = poly_g(p, make_float2(__fsub_rn(v.x, m.x), __fsub_rn(v.y, m.y)));
    mine[n] = g;
    gr = __fadd_rn(gr, g.x);
    gi = __fadd_rn(gi, g.y);
  }
  gr = wave_sum(gr);
  gi = wave_sum(gi);
  if (GROUP) {
    float* r3 = red + CUM_RED;
    if (lane == 0) { r3[wave] = gr; r3[FR_WAVES + wave] = gi; }
    __syncthreads();
    gr = red_sum(r3);
    gi = red_sum(r3 + FR_WAVES);
  }

  // pass four: the mean removal's two terms, and out.  A frame whose P the forward refuses is NaN throughout.
  const float nan = nanf("");
  const float cr = al.ok ? __fsub_rn(__fdiv_rn(gm.x, flen), __fdiv_rn(gr, flen)) : nan;
  const float ci = al.ok ? __fsub_rn(__fdiv_rn(gm.y, flen), __fdiv_rn(gi, flen)) : nan;
  for (int n = first; n < len; n += stride) {
    const float2 g = mine[n];
    store_sample(dst, len, a.planar, n, make_float2(__fadd_rn(g.x, cr), __fadd_rn(g.y, ci)));
  }
}

}  // namespace

extern "C" int iq_frames_cumulants_bwd(const float* x, const float* dscore, const float* dfeat, float* dx, int n_frames, int len,
                                       const iq_cumulants_t* par, iq_stream_t stream) {
  // nothing is launched and no device pointer dereferenced before the refusals are through
  if (!x || !dx || !par || (!dscore && !dfeat)) return IQ_ERR_ARG;
  if (len < 1 || (par->planar & ~1) || par->n_classes < 0) return IQ_ERR_ARG;
  if (par->n_classes > 0 && (!par->mu || !par->w)) return IQ_ERR_ARG;
  if (par->n_classes == 0 && dscore) return IQ_ERR_ARG;
  if (((uintptr_t)x | (uintptr_t)dx) & (par->planar ? 3 : 7)) return IQ_ERR_ARG;      // interleaved frames move as (I, Q) pairs
  if (((uintptr_t)dscore | (uintptr_t)dfeat | (uintptr_t)par->sigma2 | (uintptr_t)par->mu | (uintptr_t)par->w |
       (uintptr_t)par->bias) & 3)
    return IQ_ERR_ARG;
  if (par->n_classes > CUM_MAX_CLASSES || !frame_fits(len)) return IQ_ERR_UNSUPPORTED;
  if (n_frames <= 0) return IQ_OK;
  const int C = par->n_classes;
  if ((long)n_frames * (C > CUM_MOMS ? C : CUM_MOMS) > INT32_MAX) return IQ_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  CumBwdArgs a = {};
  a.x = x; a.dscore = dscore; a.dfeat = dfeat; a.sigma2 = par->sigma2; a.mu = par->mu; a.w = par->w; a.dx = dx;
  a.n_frames = n_frames; a.len = len; a.n_classes = C; a.planar = par->planar;
  IQ_PROF(IQ_FAM_MISC, st);
  const double bytes = (double)n_frames * (len * 16.0 + (dscore ? C * 4.0 : 0.0) + (dfeat ? 40.0 : 0.0));
  // per symbol 2 + 43 + 17 as the forward, 104 for g_n (z and its powers 34, the four k 20, the seven products and sums 50), 2 for
  // its sum and 2 on the way out; per frame about 400 for the algebra both ways and at most 40 per class
  const double flops = (double)n_frames * (len * 170.0 + 400.0 + (dscore ? C * 40.0 : 0.0));
  if (len <= CUM_WAVE_LEN) {
    IQ_PROF_K(bytes, flops, "frames_cumulants_bwd_kernel<false>");
    launch_frames(frames_cumulants_bwd_kernel<false>, dim3((unsigned)((n_frames + FR_WAVES - 1) / FR_WAVES)),
                  (size_t)FR_WAVES * len * sizeof(float2), st, a);
  } else {
    IQ_PROF_K(bytes, flops, "frames_cumulants_bwd_kernel<true>");
    launch_frames(frames_cumulants_bwd_kernel<true>, dim3((unsigned)n_frames), (size_t)len * sizeof(float2), st, a);
  }
  return iq_launch_status();
}
