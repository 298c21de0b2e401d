// Gradients of the two likelihood classifiers with respect to the frame (iq_frames_likelihood_bwd, iq_frames_likelihood_em_bwd,
// include/iqvit.h): dx = sum over the classes and hypotheses of w (-2 q) (y - m), m the soft symbol decision sum_k pi_k p_k under
// the hypothesis.  The definition, with every rounding, is in the header.
//
// The gradient at symbol n needs sample n and the forward's per-(frame, class) results, nothing else: one workgroup of FR_THREADS
// per (frame, block of LB_BLOCK = 512 symbols), wave w of it the 128 symbols behind blk * 512 + w * 128, a lane two of them (n and
// n + 64: one LDS read of a point serves both, as in likelihood.hip).  A lane keeps its two dx in registers over all classes and
// hypotheses, c ascending, then t ascending: no cross-lane reduction, no atomics, no workspace, and a symbol's dx depends on
// neither n_frames, the frame's position nor len.  Work per workgroup is uniform (every workgroup walks every class), so the
// classes go in their own order.
//
// The points sit in LDS and are read at one address by the whole wave (a broadcast: no bank conflict).  Likelihood variant: the
// table up to the end of its last class, scaled once by the frame's gain (16 KB at most); one barrier.  EM variant: p_k = h s_k
// differs from class to class, so each class with a weight is staged between two barriers.  Everything that decides whether a
// class, a hypothesis or a barrier is skipped (dloglik, the share, best_rot, h, v) is read at one address by the whole workgroup.
// Per symbol two sweeps over k by the forward's instructions: the minimum of d_k, then e_k = exp2(q2 (d_min - d_k)) with S and
// the two point-sums beside it; one division per symbol.
//
// Indices.  LDS: pts[k], k < n_pts <= LB_MAX_POINTS (likelihood), k < M <= LB_MAX_POINTS (EM).  Memory: frame fi at x + fi 2 len
// (long), sample n < len (every load and store is behind n < len); points at k < n_pts = max(offset + count) <= LB_MAX_POINTS
// (check); rot at 2 r + {0, 1}, r < R, with best_rot[oc] held to [0, R) before it is used; dloglik, loglik, best_rot, v at
// oc = fi C + c; rot_ll at oc R + r; h at 2 oc + {0, 1}; sigma2, gain at fi.
#include <math.h>

#include "frames.h"
#include "iqvit.h"
#include "prof.h"

namespace {

constexpr int LB_MAX_CLASSES = 64, LB_MAX_ROT = 256, LB_MAX_POINTS = 2048;
constexpr int LB_BLOCK = 2 * FR_THREADS;                   // symbols per workgroup
constexpr float LB_LOG2E = 1.44269504088896340736f;
constexpr float LB_MIN_NORMAL = 1.17549435e-38f;           // 2^-126

struct LbClass {
  int offset, count;
};
struct LikBwdArgs {
  const float* x;
  const float* sigma2;
  const float* gain;
  const float* points;
  const float* rot;
  const float* dloglik;
  const float* loglik;
  const float* rot_ll;
  const int* best_rot;
  float* dx;
  int n_frames, len, n_classes, n_rot, planar, mode, n_blocks, n_pts;
  LbClass cls[LB_MAX_CLASSES];
};
struct EmBwdArgs {
  const float* x;
  const float* points;
  const float* dloglik;
  const float* h;
  const float* v;
  float* dx;
  int n_frames, len, n_classes, planar, n_blocks;
  LbClass cls[LB_MAX_CLASSES];
};

// the forward's tests of its data (likelihood.hip, likelihood_em.hip)
__device__ __forceinline__ bool lb_variance_ok(float s2) { return s2 > 0.f && s2 < INFINITY; }
__device__ __forceinline__ bool lb_state_ok(float hr, float hi, float v) {
  return fabsf(hr) < INFINITY && fabsf(hi) < INFINITY && v >= LB_MIN_NORMAL && v < INFINITY;
}

__device__ __forceinline__ float lb_dist2(float2 y, float2 p) {
  const float dr = __fsub_rn(y.x, p.x), di = __fsub_rn(y.y, p.y);
  return fmaf(di, di, __fmul_rn(dr, dr));
}

// The soft decisions m of a symbol pair under the points pk[0 .. M): d_min, then S and the point-sums, then one division each.
__device__ __forceinline__ void soft_pair(const float2* pk, int M, float q2, float2 y0, float2 y1, float2& m0, float2& m1) {
  float d0 = INFINITY, d1 = INFINITY;
#pragma unroll 4
  for (int k = 0; k < M; ++k) {
    const float2 p = pk[k];
    d0 = fminf(d0, lb_dist2(y0, p));
    d1 = fminf(d1, lb_dist2(y1, p));
  }
  float S0 = 0.f, Wr0 = 0.f, Wi0 = 0.f, S1 = 0.f, Wr1 = 0.f, Wi1 = 0.f;
#pragma unroll 4
  for (int k = 0; k < M; ++k) {
    const float2 p = pk[k];
    const float e0 = __builtin_amdgcn_exp2f(__fmul_rn(q2, __fsub_rn(d0, lb_dist2(y0, p))));
    const float e1 = __builtin_amdgcn_exp2f(__fmul_rn(q2, __fsub_rn(d1, lb_dist2(y1, p))));
    S0 = __fadd_rn(S0, e0);       S1 = __fadd_rn(S1, e1);
    Wr0 = fmaf(e0, p.x, Wr0);     Wr1 = fmaf(e1, p.x, Wr1);
    Wi0 = fmaf(e0, p.y, Wi0);     Wi1 = fmaf(e1, p.y, Wi1);
  }
  const float r0 = __fdiv_rn(1.f, S0), r1 = __fdiv_rn(1.f, S1);
  m0 = make_float2(__fmul_rn(Wr0, r0), __fmul_rn(Wi0, r0));
  m1 = make_float2(__fmul_rn(Wr1, r1), __fmul_rn(Wi1, r1));
}

// this lane's two symbols of the workgroup's block, and whether the frame has them
struct LbLane {
  int n0, n1;
  bool has0, has1;
};
__device__ __forceinline__ LbLane lb_lane(int blk, int len) {
  const int tid = threadIdx.x, lane = tid & (IQ_WAVE - 1), wave = tid >> 6;
  LbLane l;
  l.n0 = blk * LB_BLOCK + wave * 2 * IQ_WAVE + lane;       // < n_blocks * 512 <= len + 511: no overflow (len * 8 <= 64 KB)
  l.n1 = l.n0 + IQ_WAVE;
  l.has0 = l.n0 < len;
  l.has1 = l.n1 < len;
  return l;
}

__global__ __launch_bounds__(FR_THREADS) void frames_likelihood_bwd_kernel(LikBwdArgs a) {
  __shared__ float2 pts[LB_MAX_POINTS];
  const int tid = threadIdx.x;
  const int len = a.len, R = a.n_rot, C = a.n_classes;
  const long fi = blockIdx.x / (unsigned)a.n_blocks;
  const LbLane l = lb_lane((int)(blockIdx.x % (unsigned)a.n_blocks), len);
  const float* src = a.x + fi * 2 * len;
  float* dst = a.dx + fi * 2 * len;
  const float s2 = a.sigma2[fi];
  if (!lb_variance_ok(s2)) {                               // the whole workgroup leaves
    const float2 nan2 = make_float2(nanf(""), nanf(""));
    if (l.has0) store_sample(dst, len, a.planar, l.n0, nan2);
    if (l.has1) store_sample(dst, len, a.planar, l.n1, nan2);
    return;
  }
  const float q = __fdiv_rn(1.f, s2), q2 = __fmul_rn(q, LB_LOG2E), m2q = __fmul_rn(-2.f, q);
  const float g = a.gain ? a.gain[fi] : 1.f;
  const float2* table = reinterpret_cast<const float2*>(a.points);
  for (int k = tid; k < a.n_pts; k += FR_THREADS) {
    const float2 p = table[k];
    pts[k] = make_float2(__fmul_rn(g, p.x), __fmul_rn(g, p.y));
  }
  __syncthreads();
  if (!l.has0) return;                                     // (no barrier below)

  const float2 zero = make_float2(0.f, 0.f);
  const float2 u0 = load_sample(src, len, a.planar, l.n0), u1 = l.has1 ? load_sample(src, len, a.planar, l.n1) : zero;
  const float inv_r = __fdiv_rn(1.f, (float)R);
  float2 g0 = zero, g1 = zero;
  for (int c = 0; c < C; ++c) {
    const long oc = fi * C + c;
    const float dl = a.dloglik[oc];
    if (dl == 0.f) continue;                               // nobody asked about this class: not even its NaNs are read
    const float2* pk = pts + a.cls[c].offset;
    const int M = a.cls[c].count;
    int r0 = 0, r1 = R;
    float ll = 0.f;
    bool lost = false;
    if (a.mode == IQ_LIK_MAX) {
      r0 = a.best_rot[oc];
      r1 = r0 + 1;
      lost = r0 < 0 || r0 >= R;                            // (-1: the forward refused the frame; anything else is not a rotation)
    } else {
      ll = a.loglik[oc];
    }
    if (lost) {
      g0 = make_float2(nanf(""), nanf(""));
      g1 = g0;
      continue;
    }
#pragma unroll 1
    for (int r = r0; r < r1; ++r) {
      float w = dl;
      if (a.mode == IQ_LIK_MEAN) {
        const float share = __builtin_amdgcn_exp2f(__fmul_rn(LB_LOG2E, __fsub_rn(a.rot_ll[oc * R + r], ll)));
        w = __fmul_rn(__fmul_rn(dl, share), inv_r);
      }
      if (w == 0.f) continue;
      const float cr = a.rot[2 * r], sr = a.rot[2 * r + 1];
      const float2 y0 = make_float2(fmaf(cr, u0.x, __fmul_rn(sr, u0.y)), fmaf(cr, u0.y, -__fmul_rn(sr, u0.x)));
      const float2 y1 = make_float2(fmaf(cr, u1.x, __fmul_rn(sr, u1.y)), fmaf(cr, u1.y, -__fmul_rn(sr, u1.x)));
      float2 m0, m1;
      soft_pair(pk, M, q2, y0, y1, m0, m1);
      const float wq = __fmul_rn(w, m2q);
      const float2 t0 = rotate(make_float2(__fmul_rn(wq, __fsub_rn(y0.x, m0.x)), __fmul_rn(wq, __fsub_rn(y0.y, m0.y))), cr, sr);
      const float2 t1 = rotate(make_float2(__fmul_rn(wq, __fsub_rn(y1.x, m1.x)), __fmul_rn(wq, __fsub_rn(y1.y, m1.y))), cr, sr);
      g0 = make_float2(__fadd_rn(g0.x, t0.x), __fadd_rn(g0.y, t0.y));
      g1 = make_float2(__fadd_rn(g1.x, t1.x), __fadd_rn(g1.y, t1.y));
    }
  }
  store_sample(dst, len, a.planar, l.n0, g0);
  if (l.has1) store_sample(dst, len, a.planar, l.n1, g1);
}

__global__ __launch_bounds__(FR_THREADS) void frames_likelihood_em_bwd_kernel(EmBwdArgs a) {
  __shared__ float2 pts[LB_MAX_POINTS];
  const int tid = threadIdx.x;
  const int len = a.len, C = a.n_classes;
  const long fi = blockIdx.x / (unsigned)a.n_blocks;
  const LbLane l = lb_lane((int)(blockIdx.x % (unsigned)a.n_blocks), len);
  const float* src = a.x + fi * 2 * len;
  float* dst = a.dx + fi * 2 * len;
  const float2 zero = make_float2(0.f, 0.f);
  const float2 y0 = l.has0 ? load_sample(src, len, a.planar, l.n0) : zero, y1 = l.has1 ? load_sample(src, len, a.planar, l.n1) : zero;
  float2 g0 = zero, g1 = zero;
  for (int c = 0; c < C; ++c) {                            // dl, h and v are the same in all threads: so is every branch around a barrier
    const long oc = fi * C + c;
    const float dl = a.dloglik[oc];
    if (dl == 0.f) continue;
    const float hr = a.h[2 * oc], hi = a.h[2 * oc + 1], v = a.v[oc];
    if (!lb_state_ok(hr, hi, v)) {                         // a dead (frame, class) somebody asked about
      g0 = make_float2(nanf(""), nanf(""));
      g1 = g0;
      continue;
    }
    const int M = a.cls[c].count;
    const float2* table = reinterpret_cast<const float2*>(a.points) + a.cls[c].offset;
    __syncthreads();                                       // the reads of the class before are done
    for (int k = tid; k < M; k += FR_THREADS) pts[k] = rotate(table[k], hr, hi);
    __syncthreads();
    if (!l.has0) continue;                                 // (a wave behind the frame's end keeps to the barriers)
    const float q = __fdiv_rn(1.f, v), q2 = __fmul_rn(q, LB_LOG2E), wq = __fmul_rn(dl, __fmul_rn(-2.f, q));
    float2 m0, m1;
    soft_pair(pts, M, q2, y0, y1, m0, m1);
    g0 = make_float2(fmaf(wq, __fsub_rn(y0.x, m0.x), g0.x), fmaf(wq, __fsub_rn(y0.y, m0.y), g0.y));
    g1 = make_float2(fmaf(wq, __fsub_rn(y1.x, m1.x), g1.x), fmaf(wq, __fsub_rn(y1.y, m1.y), g1.y));
  }
  if (l.has0) store_sample(dst, len, a.planar, l.n0, g0);
  if (l.has1) store_sample(dst, len, a.planar, l.n1, g1);
}

// The class list of both entries: -> IQ_OK, IQ_ERR_ARG, or IQ_ERR_UNSUPPORTED where a class ends behind the table's limit
int check_classes(const iq_synth_class_t* classes, int n_classes) {
  const int nc = n_classes < LB_MAX_CLASSES ? n_classes : LB_MAX_CLASSES;
  bool large = false;
  for (int i = 0; i < nc; ++i) {
    const iq_synth_class_t& c = classes[i];
    if (c.kind != 0 || c.count < 1 || c.offset < 0 || c.offset > INT32_MAX - c.count) return IQ_ERR_ARG;
    large = large || c.offset + c.count > LB_MAX_POINTS;
  }
  return large ? IQ_ERR_UNSUPPORTED : IQ_OK;
}

// -> the number of points the classes reach
int copy_classes(LbClass* out, const iq_synth_class_t* classes, int n_classes, double* points) {
  int end = 0;
  *points = 0;
  for (int i = 0; i < n_classes; ++i) {
    out[i] = LbClass{classes[i].offset, classes[i].count};
    *points += classes[i].count;
    end = out[i].offset + out[i].count > end ? out[i].offset + out[i].count : end;
  }
  return end;
}

}  // namespace

extern "C" int iq_frames_likelihood_bwd(const float* x, const float* sigma2, const float* dloglik, const float* loglik,
                                        const float* rot_ll, const int* best_rot, float* dx, int n_frames, int len,
                                        const iq_likelihood_t* par, iq_stream_t stream) {
  // nothing is launched and no device pointer dereferenced before the refusals are through
  if (!x || !sigma2 || !dloglik || !dx || !par || !par->points || !par->classes || !par->rot) return IQ_ERR_ARG;
  if (len < 1 || par->n_classes < 1 || par->n_rot < 1) return IQ_ERR_ARG;
  if ((par->planar & ~1) || (par->mode != IQ_LIK_MAX && par->mode != IQ_LIK_MEAN)) return IQ_ERR_ARG;
  if (par->mode == IQ_LIK_MAX ? !best_rot : (!loglik || !rot_ll)) return IQ_ERR_ARG;
  if (((uintptr_t)x | (uintptr_t)dx) & (par->planar ? 3 : 7)) return IQ_ERR_ARG;      // interleaved frames move as (I, Q) pairs
  if ((uintptr_t)par->points & 7) return IQ_ERR_ARG;                                  // so do the points
  if (((uintptr_t)sigma2 | (uintptr_t)dloglik | (uintptr_t)loglik | (uintptr_t)rot_ll | (uintptr_t)best_rot | (uintptr_t)par->rot |
       (uintptr_t)par->gain) & 3)
    return IQ_ERR_ARG;
  const int cc = check_classes(par->classes, par->n_classes);
  if (cc == IQ_ERR_ARG) return cc;
  if (cc != IQ_OK || par->n_classes > LB_MAX_CLASSES || par->n_rot > LB_MAX_ROT || !frame_fits(len)) return IQ_ERR_UNSUPPORTED;
  if (n_frames <= 0) return IQ_OK;
  const int n_blocks = (len + LB_BLOCK - 1) / LB_BLOCK;
  if ((long)n_frames * n_blocks > INT32_MAX) return IQ_ERR_UNSUPPORTED;               // the grid's x extent
  hipStream_t st = (hipStream_t)stream;
  LikBwdArgs a = {};
  a.x = x; a.sigma2 = sigma2; a.gain = par->gain; a.points = par->points; a.rot = par->rot;
  a.dloglik = dloglik; a.loglik = loglik; a.rot_ll = rot_ll; a.best_rot = best_rot; a.dx = dx;
  a.n_frames = n_frames; a.len = len; a.n_classes = par->n_classes; a.n_rot = par->n_rot; a.planar = par->planar; a.mode = par->mode;
  a.n_blocks = n_blocks;
  double points;
  a.n_pts = copy_classes(a.cls, par->classes, par->n_classes, &points);
  {
  IQ_PROF(IQ_FAM_MISC, st);
  const double evals = (double)n_frames * len * points * (par->mode == IQ_LIK_MEAN ? par->n_rot : 1);   // at most: zero weights are skipped
  IQ_PROF_K((double)n_frames * (len * 16.0 + par->n_classes * 8.0), evals * 16.0, "frames_likelihood_bwd_kernel");
  frames_likelihood_bwd_kernel<<<dim3((unsigned)(n_frames * n_blocks)), FR_THREADS, 0, st>>>(a);
  }
  return iq_launch_status();
}

extern "C" int iq_frames_likelihood_em_bwd(const float* x, const float* dloglik, const float* h, const float* v, float* dx,
                                           int n_frames, int len, const iq_likelihood_em_t* par, iq_stream_t stream) {
  if (!x || !dloglik || !h || !v || !dx || !par || !par->points || !par->classes) return IQ_ERR_ARG;
  if (len < 1 || par->n_classes < 1 || (par->planar & ~1)) return IQ_ERR_ARG;
  if (((uintptr_t)x | (uintptr_t)dx) & (par->planar ? 3 : 7)) return IQ_ERR_ARG;      // interleaved frames move as (I, Q) pairs
  if (((uintptr_t)par->points | (uintptr_t)h) & 7) return IQ_ERR_ARG;                 // so do the points and h
  if (((uintptr_t)dloglik | (uintptr_t)v) & 3) return IQ_ERR_ARG;
  const int cc = check_classes(par->classes, par->n_classes);
  if (cc == IQ_ERR_ARG) return cc;
  if (cc != IQ_OK || par->n_classes > LB_MAX_CLASSES || !frame_fits(len)) return IQ_ERR_UNSUPPORTED;
  if (n_frames <= 0) return IQ_OK;
  const int n_blocks = (len + LB_BLOCK - 1) / LB_BLOCK;
  if ((long)n_frames * n_blocks > INT32_MAX) return IQ_ERR_UNSUPPORTED;               // the grid's x extent
  hipStream_t st = (hipStream_t)stream;
  EmBwdArgs a = {};
  a.x = x; a.points = par->points; a.dloglik = dloglik; a.h = h; a.v = v; a.dx = dx;
  a.n_frames = n_frames; a.len = len; a.n_classes = par->n_classes; a.planar = par->planar; a.n_blocks = n_blocks;
  double points;
  (void)copy_classes(a.cls, par->classes, par->n_classes, &points);
  {
  IQ_PROF(IQ_FAM_MISC, st);
  IQ_PROF_K((double)n_frames * (len * 16.0 + par->n_classes * 16.0), (double)n_frames * len * points * 16.0,
            "frames_likelihood_em_bwd_kernel");
  frames_likelihood_em_bwd_kernel<<<dim3((unsigned)(n_frames * n_blocks)), FR_THREADS, 0, st>>>(a);
  }
  return iq_launch_status();
}
