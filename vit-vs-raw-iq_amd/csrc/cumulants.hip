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

#include "cumulants_common.h"
#include "frames.h"
#include "iqvit.h"
#include "prof.h"

#pragma clang fp contract(off)       // a product and a sum are fused where fmaf says so and nowhere else

namespace {

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

template <bool GROUP>
__global__ __launch_bounds__(FR_THREADS) void frames_cumulants_kernel(CumArgs a) {
  extern __shared__ float2 keep[];
  __shared__ float red[CUM_RED];
  const int tid = threadIdx.x, lane = tid & (IQ_WAVE - 1), wave = tid >> 6;
  const int len = a.len, C = a.n_classes;
  const long fi = GROUP ? (long)blockIdx.x : (long)blockIdx.x * FR_WAVES + wave;
  if (!GROUP && fi >= a.n_frames) return;                  // (the wave route holds no barrier)
  const int first = GROUP ? tid : lane, stride = GROUP ? FR_THREADS : IQ_WAVE;
  float2* mine = keep + (GROUP ? 0 : wave * len);
  const float* src = a.x + fi * 2 * len;

  // pass one: the mean; pass two: the 17 central sums (cumulants_common.h, which the backward runs too)
  const float2 m = cum_mean<GROUP>(src, len, a.planar, mine, red, first, stride, lane, wave);
  const float mr = m.x, mi = m.y;
  float s[CUM_SUMS];
  cum_sums<GROUP>(mine, len, m, red, first, stride, lane, wave, s);
  if (GROUP && wave != 0) return;                          // (behind the last barrier)
  cum_moments<GROUP>(red, len, s);

  // the algebra of the header, on the same numbers in every lane
  const CumAlgebra al = cum_algebra(m, s, a.sigma2 ? a.sigma2[fi] : 0.f);
  const float P = al.P;
  const bool ok = al.ok;
  const float nan = nanf("");
  const float* f = al.f;

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
