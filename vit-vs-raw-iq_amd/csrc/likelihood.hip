// Likelihood classifier (iq_frames_likelihood, include/iqvit.h): the log-likelihood of every frame under every candidate
// constellation, over a table of carrier rotations, and the decision.  The definition, with every rounding, is in the header.
//
// One workgroup of FR_THREADS per (frame, class); all R rotations of the pair run inside it, so that the maximum / mean over r
// needs neither a workspace nor an atomic.  The work of a pair is R len M_c evaluations and M_c runs from 2 to 256 in the
// project's table: the host orders the classes by descending M_c and the grid walks (class in that order, frame), so the long
// workgroups start first and the short ones fill the tail behind them.
//
// Plain VALU, bound by the exponential.  Wave w takes the rotations r = w, w + 4, ...; lane l takes the symbols n = l, l + 64, ...,
// two at a time (n and n + 64: one LDS read of a point serves both).  The class's points, scaled by the frame's gain, sit in LDS
// as (re, im) pairs and are read at one address by the whole wave (a broadcast: no bank conflict).  Per symbol two passes over k:
// the minimum of d_k, then the sum of exp2(q2 (d_min - d_k)) with d_k recomputed by the same instructions (so d_k - d_min is
// exactly 0 at the minimum and never negative).  The sum over the symbols of a rotation never leaves its wave: the lane's chain,
// then the butterfly; lane 0 writes L[r] to LDS (and to rot_ll).  One barrier, then thread 0 walks L[0 .. R) in order.  No
// dynamic LDS: 2048 points (16 KB) + 256 sums (1 KB).
//
// Indices.  LDS: pts[k], k < M <= LIK_MAX_POINTS; Lr[r], r < R <= LIK_MAX_ROT.  Memory: frame fi at x + fi 2 len (long), sample n < len;
// points at offset + k < offset + count <= LIK_MAX_POINTS (check); rot at 2 r + {0, 1}, r < R; loglik, best_rot at fi C + c; rot_ll at
// (fi C + c) R + r; sigma2, gain, pred at fi.
#include <math.h>

#include "frames.h"
#include "iqvit.h"
#include "prof.h"

namespace {

constexpr int LIK_MAX_CLASSES = 64, LIK_MAX_ROT = 256, LIK_MAX_POINTS = 2048;
constexpr float LIK_LOG2E = 1.44269504088896340736f, LIK_LN2 = 0.69314718055994530942f;

struct LikClass {
  int offset, count;
};
struct LikArgs {
  const float* x;
  const float* sigma2;
  const float* gain;
  const float* points;
  const float* rot;
  float* loglik;
  float* rot_ll;
  int* best_rot;
  int n_frames, len, n_classes, n_rot, planar, mode;
  LikClass cls[LIK_MAX_CLASSES];
  unsigned char order[LIK_MAX_CLASSES];                    // the classes by descending count (ties: ascending index)
};

// sigma2 is data: a frame whose variance is not a positive finite number gets NaN outputs
__device__ __forceinline__ bool variance_ok(float s2) { return s2 > 0.f && s2 < INFINITY; }

__device__ __forceinline__ float dist2(float yr, float yi, float2 p) {
  const float dr = __fsub_rn(yr, p.x), di = __fsub_rn(yi, p.y);
  return fmaf(di, di, __fmul_rn(dr, dr));
}

// l_n of the header from the minimum and the sum of one symbol
__device__ __forceinline__ float symbol_ll(float q, float dmin, float sum, float inv_m) {
  return fmaf(-q, dmin, __fmul_rn(LIK_LN2, __builtin_amdgcn_logf(__fmul_rn(sum, inv_m))));
}

__global__ __launch_bounds__(FR_THREADS) void frames_likelihood_kernel(LikArgs a) {
  __shared__ float2 pts[LIK_MAX_POINTS];
  __shared__ float Lr[LIK_MAX_ROT];
  const int tid = threadIdx.x, lane = tid & (IQ_WAVE - 1), wave = tid >> 6;
  const int len = a.len, R = a.n_rot, C = a.n_classes;
  const long fi = blockIdx.x % (unsigned)a.n_frames;
  const int c = a.order[blockIdx.x / (unsigned)a.n_frames];
  const int M = a.cls[c].count;
  const float s2 = a.sigma2[fi];
  const long oc = fi * C + c;
  if (!variance_ok(s2)) {                                  // the whole workgroup leaves: no barrier is skipped by a part of it
    const float nan = nanf("");
    if (tid == 0) {
      a.loglik[oc] = nan;
      if (a.best_rot) a.best_rot[oc] = -1;
    }
    if (a.rot_ll)
      for (int r = tid; r < R; r += FR_THREADS) a.rot_ll[oc * R + r] = nan;
    return;
  }
  const float q = __fdiv_rn(1.f, s2), q2 = __fmul_rn(q, LIK_LOG2E);
  const float g = a.gain ? a.gain[fi] : 1.f;
  const float inv_m = __fdiv_rn(1.f, (float)M);
  const float2* table = reinterpret_cast<const float2*>(a.points) + a.cls[c].offset;
  for (int k = tid; k < M; k += FR_THREADS) {
    const float2 p = table[k];
    pts[k] = make_float2(__fmul_rn(g, p.x), __fmul_rn(g, p.y));
  }
  __syncthreads();

  const float* src = a.x + fi * 2 * len;
  for (int r = wave; r < R; r += FR_WAVES) {
    const float cr = a.rot[2 * r], sr = a.rot[2 * r + 1];
    float acc = 0.f;
#pragma unroll 1
    for (int n0 = lane; n0 < len; n0 += 2 * IQ_WAVE) {
      const int n1 = n0 + IQ_WAVE;
      const bool two = n1 < len;
      const float2 u0 = load_sample(src, len, a.planar, n0);
      const float2 u1 = two ? load_sample(src, len, a.planar, n1) : make_float2(0.f, 0.f);
      const float y0r = fmaf(cr, u0.x, __fmul_rn(sr, u0.y)), y0i = fmaf(cr, u0.y, -__fmul_rn(sr, u0.x));
      const float y1r = fmaf(cr, u1.x, __fmul_rn(sr, u1.y)), y1i = fmaf(cr, u1.y, -__fmul_rn(sr, u1.x));
      float m0 = INFINITY, m1 = INFINITY;
#pragma unroll 4
      for (int k = 0; k < M; ++k) {
        const float2 p = pts[k];
        m0 = fminf(m0, dist2(y0r, y0i, p));
        m1 = fminf(m1, dist2(y1r, y1i, p));
      }
      float e0 = 0.f, e1 = 0.f;
#pragma unroll 4
      for (int k = 0; k < M; ++k) {
        const float2 p = pts[k];
        e0 = __fadd_rn(e0, __builtin_amdgcn_exp2f(__fmul_rn(q2, __fsub_rn(m0, dist2(y0r, y0i, p)))));
        e1 = __fadd_rn(e1, __builtin_amdgcn_exp2f(__fmul_rn(q2, __fsub_rn(m1, dist2(y1r, y1i, p)))));
      }
      acc = __fadd_rn(acc, symbol_ll(q, m0, e0, inv_m));
      if (two) acc = __fadd_rn(acc, symbol_ll(q, m1, e1, inv_m));
    }
    acc = wave_sum(acc);
    if (lane == 0) {
      Lr[r] = acc;
      if (a.rot_ll) a.rot_ll[oc * R + r] = acc;
    }
  }
  __syncthreads();
  if (tid == 0) {
    float best = Lr[0];
    int at = 0;
    for (int r = 1; r < R; ++r)                            // the first largest; a NaN is never larger (nor ever beaten)
      if (Lr[r] > best) { best = Lr[r]; at = r; }
    float out = best;
    if (a.mode == IQ_LIK_MEAN) {
      float s = 0.f;
      for (int r = 0; r < R; ++r) s = __fadd_rn(s, __builtin_amdgcn_exp2f(__fmul_rn(LIK_LOG2E, __fsub_rn(Lr[r], best))));
      out = __fadd_rn(best, __fmul_rn(LIK_LN2, __builtin_amdgcn_logf(__fmul_rn(s, __fdiv_rn(1.f, (float)R)))));
    }
    a.loglik[oc] = out;
    if (a.best_rot) a.best_rot[oc] = at;
  }
}

// pred[fi] = the first class with the largest loglik; -1 for a frame whose variance is refused
__global__ __launch_bounds__(FR_THREADS) void likelihood_decide_kernel(const float* loglik, const float* sigma2, int* pred,
                                                                       int n_frames, int n_classes) {
  const long fi = (long)blockIdx.x * FR_THREADS + threadIdx.x;
  if (fi >= n_frames) return;
  const float* row = loglik + fi * n_classes;
  float best = row[0];
  int at = 0;
  for (int c = 1; c < n_classes; ++c)
    if (row[c] > best) { best = row[c]; at = c; }
  pred[fi] = variance_ok(sigma2[fi]) ? at : -1;
}

// -> IQ_OK or the refusal; nothing is launched and no device pointer dereferenced before this returns IQ_OK
int check(const float* x, const float* sigma2, const float* loglik, const float* rot_ll, const int* best_rot, const int* pred,
          int len, const iq_likelihood_t* p) {
  if (!x || !sigma2 || !loglik || !p || !p->points || !p->classes || !p->rot) return IQ_ERR_ARG;
  if (len < 1 || p->n_classes < 1 || p->n_rot < 1) return IQ_ERR_ARG;
  if ((p->planar & ~1) || (p->mode != IQ_LIK_MAX && p->mode != IQ_LIK_MEAN)) return IQ_ERR_ARG;
  if ((uintptr_t)x & (p->planar ? 3 : 7)) return IQ_ERR_ARG;         // interleaved frames move as (I, Q) pairs
  if ((uintptr_t)p->points & 7) return IQ_ERR_ARG;                   // so do the points
  if (((uintptr_t)sigma2 | (uintptr_t)loglik | (uintptr_t)rot_ll | (uintptr_t)best_rot | (uintptr_t)pred | (uintptr_t)p->rot |
       (uintptr_t)p->gain) & 3)
    return IQ_ERR_ARG;
  const int nc = p->n_classes < LIK_MAX_CLASSES ? p->n_classes : LIK_MAX_CLASSES;
  bool large = false;
  for (int i = 0; i < nc; ++i) {
    const iq_synth_class_t& c = p->classes[i];
    if (c.kind != 0 || c.count < 1 || c.offset < 0 || c.offset > INT32_MAX - c.count) return IQ_ERR_ARG;
    large = large || c.offset + c.count > LIK_MAX_POINTS;
  }
  if (large || p->n_classes > LIK_MAX_CLASSES || p->n_rot > LIK_MAX_ROT || !frame_fits(len)) return IQ_ERR_UNSUPPORTED;
  return IQ_OK;
}

}  // namespace

extern "C" int iq_frames_likelihood(const float* x, const float* sigma2, float* loglik, float* rot_ll, int* best_rot, int* pred,
                                    int n_frames, int len, const iq_likelihood_t* par, iq_stream_t stream) {
  const int rc = check(x, sigma2, loglik, rot_ll, best_rot, pred, len, par);
  if (rc != IQ_OK) return rc;
  if (n_frames <= 0) return IQ_OK;
  const int C = par->n_classes;
  if ((long)n_frames * C > INT32_MAX) return IQ_ERR_UNSUPPORTED;     // the grid's x extent
  hipStream_t st = (hipStream_t)stream;
  LikArgs a = {};
  a.x = x; a.sigma2 = sigma2; a.gain = par->gain; a.points = par->points; a.rot = par->rot;
  a.loglik = loglik; a.rot_ll = rot_ll; a.best_rot = best_rot;
  a.n_frames = n_frames; a.len = len; a.n_classes = C; a.n_rot = par->n_rot; a.planar = par->planar; a.mode = par->mode;
  double points = 0;
  for (int i = 0; i < C; ++i) {
    a.cls[i] = LikClass{par->classes[i].offset, par->classes[i].count};
    points += par->classes[i].count;
    int j = i;                                             // insertion by descending count: stable, so ties keep their order
    for (; j > 0 && a.cls[a.order[j - 1]].count < a.cls[i].count; --j) a.order[j] = a.order[j - 1];
    a.order[j] = (unsigned char)i;
  }
  {
    IQ_PROF(IQ_FAM_MISC, st);
    const double evals = (double)n_frames * len * par->n_rot * points;     // 5 + 9 operations each: the two passes
    IQ_PROF_K((double)n_frames * (len * 8.0 + C * 4.0), evals * 14.0, "frames_likelihood_kernel");
    frames_likelihood_kernel<<<dim3((unsigned)(n_frames * C)), FR_THREADS, 0, st>>>(a);
  }
  if (pred) {
    IQ_PROF(IQ_FAM_MISC, st);
    IQ_PROF_K((double)n_frames * (C + 1) * 4.0, (double)n_frames * C, "likelihood_decide_kernel");
    likelihood_decide_kernel<<<dim3((unsigned)((n_frames + FR_THREADS - 1) / FR_THREADS)), FR_THREADS, 0, st>>>(
        loglik, sigma2, pred, n_frames, C);
  }
  return iq_launch_status();
}
