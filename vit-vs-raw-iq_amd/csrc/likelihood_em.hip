// Hybrid likelihood classifier (iq_frames_likelihood_em, include/iqvit.h): per frame and candidate constellation the
// maximum-likelihood complex gain h and noise variance v by expectation-maximisation from a table of starts, the log-likelihood
// at them, and the decision with its blind SNR estimate.  The definition, with every rounding, is in the header.
//
// The shape is likelihood.hip's: one workgroup of FR_THREADS per (frame, class), the classes going out by descending size, the
// class's points in LDS read as a broadcast, lanes splitting the symbols two at a time (n and n + 64).  What differs: the state
// (h, v) changes from pass to pass, so ONE WAVE runs one EM chain -- wave w takes the starts t = w, w + 4, ... and runs all
// iters + 1 passes of a start on its own.  Every sum over the symbols is then a lane chain plus the wave's butterfly, all 64
// lanes hold the same (h, v) bit for bit (the butterfly's additions commute), and the iteration needs no workgroup barrier: there
// are two in the kernel, behind the staging and in front of the walk over the starts.  In IQ_EM_GIVEN three waves idle.
//
// LDS.  The frame is read iters + 1 times T / 4 times by each wave: it is staged once (len * 8 bytes, dynamic).  The points
// scaled by a wave's own h, p_k = h s_k, are the same for all its lanes and symbols: each wave writes them to its own table
// (M * 8 bytes per wave, dynamic) at the head of a pass -- M / 64 complex products per lane against len M / 64 evaluations --
// and reads them as a broadcast.  A wave's LDS instructions execute in order, so the table needs a wave-level fence only.
// Static: the unscaled points (16 KB), |s_k|^2 (8 KB) and the starts' results (4 KB).
//
// Per symbol two sweeps over k as in likelihood.hip: the minimum of d_k, then e_k = exp2(q2 (d_min - d_k)) with d_k recomputed by
// the same instructions.  An update pass forms the four point-sums in that second sweep and divides by S once; the last pass
// forms l_n only.  Counted in this source, not in the ISA: per evaluation 5 + (7 + exp2 + 4 fmaf) vector operations in an update
// pass against 5 + (7 + exp2) there, and five LDS dwords per point in its second sweep (p_k, s_k, ss_k: two 8-byte reads and one
// 4-byte read, each serving both symbols of the pair) against two.
//
// Indices.  LDS: pts[k], ss[k], k < M <= EM_MAX_POINTS; res*[t], t < T <= EM_MAX_STARTS; fr[n], n < len; pk[wave * M + k],
// wave < FR_WAVES, k < M: the dynamic size is len * 8 + FR_WAVES * M * 8.  Memory: frame fi at x + fi 2 len (long), sample n < len;
// points at offset + k < offset + count <= EM_MAX_POINTS (check); starts at 2 t + {0, 1}, t < T; loglik, v, best_start, v0 at
// oc = fi C + c; h, h0 at 2 oc + {0, 1}; start_ll at oc T + t; pred, snr_db at fi.
#include <math.h>

#include "frames.h"
#include "iqvit.h"
#include "prof.h"

namespace {

constexpr int EM_MAX_CLASSES = 64, EM_MAX_STARTS = 256, EM_MAX_POINTS = 2048, EM_MAX_ITERS = 4096;
constexpr size_t EM_STATIC_LDS = EM_MAX_POINTS * 12 + EM_MAX_STARTS * 16;   // pts, ss; resH, resV, resL
constexpr float EM_LOG2E = 1.44269504088896340736f, EM_LN2 = 0.69314718055994530942f;
constexpr float EM_MIN_NORMAL = 1.17549435e-38f;          // 2^-126
constexpr float EM_LOG2PI = 1.65149612947231879804f, EM_TEN_LOG10_2 = 3.01029995663981195214f;

struct EmClass {
  int offset, count;
};
struct EmArgs {
  const float* x;
  const float* points;
  const float* starts;
  const float* h0;
  const float* v0;
  float* loglik;
  float* h;
  float* v;
  int* best_start;
  float* start_ll;
  int n_frames, len, n_classes, n_starts, iters, planar, mode;
  float f0, floor;
  EmClass cls[EM_MAX_CLASSES];
  unsigned char order[EM_MAX_CLASSES];                     // the classes by descending count (ties: ascending index)
};

// (v normal: the raw v_log_f32 and the division take a subnormal for zero, and Lambda would be +inf)
__device__ __forceinline__ bool state_ok(float hr, float hi, float v) {
  return fabsf(hr) < INFINITY && fabsf(hi) < INFINITY && v >= EM_MIN_NORMAL && v < INFINITY;
}

__device__ __forceinline__ float em_dist2(float2 y, float2 p) {
  const float dr = __fsub_rn(y.x, p.x), di = __fsub_rn(y.y, p.y);
  return fmaf(di, di, __fmul_rn(dr, dr));
}

// what one wave wrote to its own table is read by its other lanes: the wave's LDS instructions execute in order; this keeps the
// compiler from moving one across
__device__ __forceinline__ void wave_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// d_min of one symbol pair over the wave's scaled points
__device__ __forceinline__ void em_minima(const float2* pk, int M, float2 y0, float2 y1, float& m0, float& m1) {
  m0 = INFINITY;
  m1 = INFINITY;
#pragma unroll 4
  for (int k = 0; k < M; ++k) {
    const float2 p = pk[k];
    m0 = fminf(m0, em_dist2(y0, p));
    m1 = fminf(m1, em_dist2(y1, p));
  }
}

// The update sums (Ar, Ai, Bq, V) of the header at the state whose scaled points are in pk, complete in every lane.
__device__ __forceinline__ void em_update_pass(const float2* fr, int len, const float2* pk, const float2* pts, const float* ss, int M,
                                               float q2, int lane, float& Ar, float& Ai, float& Bq, float& V) {
  Ar = 0.f; Ai = 0.f; Bq = 0.f; V = 0.f;
#pragma unroll 1
  for (int n0 = lane; n0 < len; n0 += 2 * IQ_WAVE) {
    const int n1 = n0 + IQ_WAVE;
    const bool two = n1 < len;
    const float2 y0 = fr[n0], y1 = two ? fr[n1] : make_float2(0.f, 0.f);
    float m0, m1;
    em_minima(pk, M, y0, y1, m0, m1);
    float S0 = 0.f, Wr0 = 0.f, Wi0 = 0.f, B0 = 0.f, V0 = 0.f, S1 = 0.f, Wr1 = 0.f, Wi1 = 0.f, B1 = 0.f, V1 = 0.f;
#pragma unroll 2
    for (int k = 0; k < M; ++k) {
      const float2 p = pk[k], s = pts[k];
      const float w = ss[k];
      const float d0 = em_dist2(y0, p), d1 = em_dist2(y1, p);
      const float e0 = __builtin_amdgcn_exp2f(__fmul_rn(q2, __fsub_rn(m0, d0)));
      const float e1 = __builtin_amdgcn_exp2f(__fmul_rn(q2, __fsub_rn(m1, d1)));
      S0 = __fadd_rn(S0, e0);       S1 = __fadd_rn(S1, e1);
      Wr0 = fmaf(e0, s.x, Wr0);     Wr1 = fmaf(e1, s.x, Wr1);
      Wi0 = fmaf(e0, s.y, Wi0);     Wi1 = fmaf(e1, s.y, Wi1);
      B0 = fmaf(e0, w, B0);         B1 = fmaf(e1, w, B1);
      V0 = fmaf(e0, d0, V0);        V1 = fmaf(e1, d1, V1);
    }
    {
      const float r = __fdiv_rn(1.f, S0), gr = __fmul_rn(Wr0, r), gi = __fmul_rn(Wi0, r);
      Ar = fmaf(y0.y, gi, fmaf(y0.x, gr, Ar));
      Ai = fmaf(-y0.x, gi, fmaf(y0.y, gr, Ai));
      Bq = fmaf(B0, r, Bq);
      V = fmaf(V0, r, V);
    }
    if (two) {
      const float r = __fdiv_rn(1.f, S1), gr = __fmul_rn(Wr1, r), gi = __fmul_rn(Wi1, r);
      Ar = fmaf(y1.y, gi, fmaf(y1.x, gr, Ar));
      Ai = fmaf(-y1.x, gi, fmaf(y1.y, gr, Ai));
      Bq = fmaf(B1, r, Bq);
      V = fmaf(V1, r, V);
    }
  }
  Ar = wave_sum(Ar); Ai = wave_sum(Ai); Bq = wave_sum(Bq); V = wave_sum(V);
}

// L of the header (the last pass), complete in every lane.
__device__ __forceinline__ float em_last_pass(const float2* fr, int len, const float2* pk, int M, float q, float q2, float inv_m,
                                              int lane) {
  float acc = 0.f;
#pragma unroll 1
  for (int n0 = lane; n0 < len; n0 += 2 * IQ_WAVE) {
    const int n1 = n0 + IQ_WAVE;
    const bool two = n1 < len;
    const float2 y0 = fr[n0], y1 = two ? fr[n1] : make_float2(0.f, 0.f);
    float m0, m1;
    em_minima(pk, M, y0, y1, m0, m1);
    float e0 = 0.f, e1 = 0.f;
#pragma unroll 4
    for (int k = 0; k < M; ++k) {
      const float2 p = pk[k];
      e0 = __fadd_rn(e0, __builtin_amdgcn_exp2f(__fmul_rn(q2, __fsub_rn(m0, em_dist2(y0, p)))));
      e1 = __fadd_rn(e1, __builtin_amdgcn_exp2f(__fmul_rn(q2, __fsub_rn(m1, em_dist2(y1, p)))));
    }
    acc = __fadd_rn(acc, fmaf(-q, m0, __fmul_rn(EM_LN2, __builtin_amdgcn_logf(__fmul_rn(e0, inv_m)))));
    if (two) acc = __fadd_rn(acc, fmaf(-q, m1, __fmul_rn(EM_LN2, __builtin_amdgcn_logf(__fmul_rn(e1, inv_m)))));
  }
  return wave_sum(acc);
}

__global__ __launch_bounds__(FR_THREADS) void frames_likelihood_em_kernel(EmArgs a) {
  __shared__ float2 pts[EM_MAX_POINTS];
  __shared__ float ss[EM_MAX_POINTS];
  __shared__ float2 resH[EM_MAX_STARTS];
  __shared__ float resV[EM_MAX_STARTS], resL[EM_MAX_STARTS];
  extern __shared__ __attribute__((aligned(16))) unsigned char em_dyn[];
  const int tid = threadIdx.x, lane = tid & (IQ_WAVE - 1), wave = tid >> 6;
  const int len = a.len, C = a.n_classes;
  const int T = a.mode == IQ_EM_GIVEN ? 1 : a.n_starts;
  const long fi = blockIdx.x % (unsigned)a.n_frames;
  const int c = a.order[blockIdx.x / (unsigned)a.n_frames];
  const int M = a.cls[c].count;
  const long oc = fi * C + c;
  float2* fr = reinterpret_cast<float2*>(em_dyn);
  float2* pk = fr + len + wave * M;

  const float2* table = reinterpret_cast<const float2*>(a.points) + a.cls[c].offset;
  for (int k = tid; k < M; k += FR_THREADS) {
    const float2 s = table[k];
    pts[k] = s;
    ss[k] = fmaf(s.y, s.y, __fmul_rn(s.x, s.x));
  }
  const float* src = a.x + fi * 2 * len;
  for (int n = tid; n < len; n += FR_THREADS) fr[n] = load_sample(src, len, a.planar, n);
  __syncthreads();

  if (wave < T) {                                          // (a wave without a start goes to the barrier below)
    float pw = 0.f;
    for (int n = lane; n < len; n += IQ_WAVE) {
      const float2 y = fr[n];
      pw = __fadd_rn(pw, fmaf(y.y, y.y, __fmul_rn(y.x, y.x)));
    }
    const float flen = (float)len;
    const float M2 = __fdiv_rn(wave_sum(pw), flen), vfloor = __fmul_rn(a.floor, M2);
    const float inv_m = __fdiv_rn(1.f, (float)M);
    for (int t = wave; t < T; t += FR_WAVES) {
      float hr, hi, v;
      if (a.mode == IQ_EM_GIVEN) {
        hr = a.h0[2 * oc];
        hi = a.h0[2 * oc + 1];
        v = a.v0[oc];
      } else {
        v = __fmul_rn(a.f0, M2);
        const float amp = __fsqrt_rn(__fsub_rn(M2, v));
        hr = __fmul_rn(amp, a.starts[2 * t]);
        hi = __fmul_rn(amp, a.starts[2 * t + 1]);
      }
      bool ok = state_ok(hr, hi, v);
      for (int pass = 0; ok && pass <= a.iters; ++pass) {  // ok, pass and iters are the same in all 64 lanes
        wave_lds_fence();                                  // the reads of the pass before are done
        for (int k = lane; k < M; k += IQ_WAVE) pk[k] = rotate(pts[k], hr, hi);
        wave_lds_fence();
        const float q = __fdiv_rn(1.f, v), q2 = __fmul_rn(q, EM_LOG2E);
        if (pass < a.iters) {
          float Ar, Ai, Bq, V;
          em_update_pass(fr, len, pk, pts, ss, M, q2, lane, Ar, Ai, Bq, V);
          hr = __fdiv_rn(Ar, Bq);
          hi = __fdiv_rn(Ai, Bq);
          const float tv = __fdiv_rn(V, flen);
          v = tv < vfloor ? vfloor : tv;                   // (a NaN tv stays)
          ok = state_ok(hr, hi, v);
        } else {
          const float L = em_last_pass(fr, len, pk, M, q, q2, inv_m, lane);
          const float lam = fmaf(-flen, __fmul_rn(EM_LN2, __fadd_rn(EM_LOG2PI, __builtin_amdgcn_logf(v))), L);
          if (lane == 0) {
            resL[t] = lam;
            resH[t] = make_float2(hr, hi);
            resV[t] = v;
          }
        }
      }
      if (!ok && lane == 0) resL[t] = nanf("");
    }
  }
  __syncthreads();
  if (a.start_ll)
    for (int t = tid; t < T; t += FR_THREADS) a.start_ll[oc * T + t] = resL[t];
  if (tid == 0) {
    float best = 0.f;
    int at = -1;
    for (int t = 0; t < T; ++t) {                          // the first largest, NaNs passed over
      const float l = resL[t];
      if (at < 0 ? l == l : l > best) { best = l; at = t; }
    }
    const float nan = nanf("");
    a.loglik[oc] = at < 0 ? nan : best;
    if (a.h) reinterpret_cast<float2*>(a.h)[oc] = at < 0 ? make_float2(nan, nan) : resH[at];
    if (a.v) a.v[oc] = at < 0 ? nan : resV[at];
    if (a.best_start) a.best_start[oc] = at;
  }
}

// pred[fi] = the first class with the largest loglik, NaNs passed over (-1: every class is NaN); snr_db of that class
__global__ __launch_bounds__(FR_THREADS) void likelihood_em_decide_kernel(const float* loglik, const float* h, const float* v, int* pred,
                                                                          float* snr_db, int n_frames, int n_classes) {
  const long fi = (long)blockIdx.x * FR_THREADS + threadIdx.x;
  if (fi >= n_frames) return;
  const float* row = loglik + fi * n_classes;
  float best = 0.f;
  int at = -1;
  for (int c = 0; c < n_classes; ++c) {
    const float l = row[c];
    if (at < 0 ? l == l : l > best) { best = l; at = c; }
  }
  if (pred) pred[fi] = at;
  if (snr_db) {
    float s = nanf("");
    if (at >= 0) {
      const long oc = fi * n_classes + at;
      const float hr = h[2 * oc], hi = h[2 * oc + 1];
      s = __fmul_rn(EM_TEN_LOG10_2, __builtin_amdgcn_logf(__fdiv_rn(fmaf(hi, hi, __fmul_rn(hr, hr)), v[oc])));
    }
    snr_db[fi] = s;
  }
}

// -> IQ_OK or the refusal; nothing is launched and no device pointer dereferenced before this returns IQ_OK
int check(const float* x, const float* loglik, const float* h, const float* v, const int* best_start, const float* start_ll,
          const int* pred, const float* snr_db, int len, const iq_likelihood_em_t* p) {
  if (!x || !loglik || !p || !p->points || !p->classes) return IQ_ERR_ARG;
  if (p->mode != IQ_EM_TABLE && p->mode != IQ_EM_GIVEN) return IQ_ERR_ARG;
  if (p->mode == IQ_EM_TABLE && (!p->starts || p->n_starts < 1)) return IQ_ERR_ARG;
  if (p->mode == IQ_EM_GIVEN && (!p->h0 || !p->v0)) return IQ_ERR_ARG;
  if (snr_db && (!h || !v)) return IQ_ERR_ARG;
  if (len < 1 || p->n_classes < 1 || p->iters < 0 || (p->planar & ~1)) return IQ_ERR_ARG;
  if (!(p->f0 > 0.f && p->f0 < 1.f) || !(p->floor >= 0.f && p->floor < INFINITY)) return IQ_ERR_ARG;
  if ((uintptr_t)x & (p->planar ? 3 : 7)) return IQ_ERR_ARG;         // interleaved frames move as (I, Q) pairs
  if (((uintptr_t)p->points | (uintptr_t)p->h0 | (uintptr_t)h) & 7) return IQ_ERR_ARG;           // so do the points and h
  if (((uintptr_t)loglik | (uintptr_t)v | (uintptr_t)best_start | (uintptr_t)start_ll | (uintptr_t)pred | (uintptr_t)snr_db |
       (uintptr_t)p->starts | (uintptr_t)p->v0) & 3)
    return IQ_ERR_ARG;
  const int nc = p->n_classes < EM_MAX_CLASSES ? p->n_classes : EM_MAX_CLASSES;
  bool large = false;
  for (int i = 0; i < nc; ++i) {
    const iq_synth_class_t& c = p->classes[i];
    if (c.kind != 0 || c.count < 1 || c.offset < 0 || c.offset > INT32_MAX - c.count) return IQ_ERR_ARG;
    large = large || c.offset + c.count > EM_MAX_POINTS;
  }
  if (large || p->n_classes > EM_MAX_CLASSES || (p->mode == IQ_EM_TABLE && p->n_starts > EM_MAX_STARTS) ||
      p->iters > EM_MAX_ITERS || !frame_fits(len))
    return IQ_ERR_UNSUPPORTED;
  return IQ_OK;
}

}  // namespace

extern "C" int iq_frames_likelihood_em(const float* x, float* loglik, float* h, float* v, int* best_start, float* start_ll, int* pred,
                                       float* snr_db, int n_frames, int len, const iq_likelihood_em_t* par, iq_stream_t stream) {
  const int rc = check(x, loglik, h, v, best_start, start_ll, pred, snr_db, len, par);
  if (rc != IQ_OK) return rc;
  if (n_frames <= 0) return IQ_OK;
  const int C = par->n_classes;
  if ((long)n_frames * C > INT32_MAX) return IQ_ERR_UNSUPPORTED;     // the grid's x extent
  hipStream_t st = (hipStream_t)stream;
  EmArgs a = {};
  a.x = x; a.points = par->points; a.starts = par->starts; a.h0 = par->h0; a.v0 = par->v0;
  a.loglik = loglik; a.h = h; a.v = v; a.best_start = best_start; a.start_ll = start_ll;
  a.n_frames = n_frames; a.len = len; a.n_classes = C; a.n_starts = par->mode == IQ_EM_GIVEN ? 1 : par->n_starts;
  a.iters = par->iters; a.planar = par->planar; a.mode = par->mode; a.f0 = par->f0; a.floor = par->floor;
  double points = 0;
  int largest = 0;
  for (int i = 0; i < C; ++i) {
    a.cls[i] = EmClass{par->classes[i].offset, par->classes[i].count};
    points += par->classes[i].count;
    largest = a.cls[i].count > largest ? a.cls[i].count : largest;
    int j = i;                                             // insertion by descending count: stable, so ties keep their order
    for (; j > 0 && a.cls[a.order[j - 1]].count < a.cls[i].count; --j) a.order[j] = a.order[j - 1];
    a.order[j] = (unsigned char)i;
  }
  {
    IQ_PROF(IQ_FAM_MISC, st);
    const double evals = (double)n_frames * len * a.n_starts * points;     // per pass: 5 + 12 (update) or 5 + 8 (last) operations
    IQ_PROF_K((double)n_frames * (len * 8.0 + C * 20.0), evals * (par->iters * 17.0 + 13.0), "frames_likelihood_em_kernel");
    const size_t lds = (size_t)len * 8 + (size_t)FR_WAVES * largest * 8;   // every workgroup gets the largest class's tables
    if (EM_STATIC_LDS + lds > 48 * 1024)                                   // (launch_frames looks at the dynamic part alone)
      (void)hipFuncSetAttribute((const void*)frames_likelihood_em_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    frames_likelihood_em_kernel<<<dim3((unsigned)(n_frames * C)), FR_THREADS, lds, st>>>(a);
  }
  if (pred || snr_db) {
    IQ_PROF(IQ_FAM_MISC, st);
    IQ_PROF_K((double)n_frames * (C + 5) * 4.0, (double)n_frames * C, "likelihood_em_decide_kernel");
    likelihood_em_decide_kernel<<<dim3((unsigned)((n_frames + FR_THREADS - 1) / FR_THREADS)), FR_THREADS, 0, st>>>(
        loglik, h, v, pred, snr_db, n_frames, C);
  }
  return iq_launch_status();
}
