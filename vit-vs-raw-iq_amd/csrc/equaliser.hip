// Blind equaliser (iq_frames_equalise / _bwd, include/iqvit.h): block constant-modulus descent of an L-tap complex filter per
// frame, and the filter.  One workgroup per frame (workgroup size, launch and the fixed-order sum of the wave sums: frames.h); the
// whole descent runs inside one launch.
//
// Plain VALU.  Thread n % 256 owns output n.  A pass over the frame (one per step, and one more for out) takes, per output, the
// window z[n + c - l], l < L, from LDS into registers, runs the fmaf chain of y[n], and -- in a step -- forms e[n] and adds
// conj(window) e[n] to the thread's 2 L gradient sums: e never leaves its thread and the window is read once.  The kernels are
// templates on L (one instance per tap count 1 .. 32, chosen on the host): the loops over l unroll fully and w, the window and
// the gradient sums stay in registers, 6 L of them and no scratch.  Then the butterflies, the wave sums to LDS, a barrier, threads
// j < 2 L each finish one component of g and step their word of w in LDS, a barrier: two barriers per step.
//
// LDS: zr [S] | zi [S] | w [2 EQ_MAX_TAPS] | red [2 EQ_MAX_TAPS + 1][FR_WAVES], S = len + 2 EQ_PAD: the frame as two planes with
// EQ_PAD zeros on either side, so that the window needs no test at the frame's edges (which is why stage_frame, which keeps the
// frame as it lies in memory, is not used).  At most 4 (2 (8192 + 64) + 64 + 260) = 67344 bytes.  Lanes read consecutive words
// of a plane: no bank conflict; w is read at one address by all lanes.
//
// Indices.  LDS window: n + c - l + EQ_PAD with 0 <= n < len, 0 <= l < L <= 32, c = L / 2 <= 16: from EQ_PAD - (L - 1 - c) >= 16 to
// len - 1 + c + EQ_PAD <= S - 17.  The adjoint's window m - c + l + EQ_PAD: from EQ_PAD - c >= 16 to len - 1 + (L - 1 - c) + EQ_PAD
// <= S - 17.  Memory: frame fi at x + fi 2 len (long), sample n < len; w, w0, w_out at (fi L + l) 2, l < L; est at 4 fi.
#include <math.h>

#include "frames.h"
#include "iqvit.h"
#include "prof.h"

namespace {

constexpr int EQ_MAX_TAPS = 32, EQ_MAX_ITERS = 4096, EQ_PAD = 32;
constexpr int EQ_SUMS = 2 * EQ_MAX_TAPS + 1;              // Re g, Im g interleaved by tap, then the sum of J

struct EqArgs {
  const float* x;       // forward: the frames; backward: dout
  float* out;           // forward: out; backward: dx
  const float* w;
  const float* w0;
  float* w_out;
  float* est;
  int len, taps, iters, planar, mode;
  float mu, modulus;
};

__host__ __device__ inline size_t eq_lds_floats(int len, bool descent) {
  return (size_t)2 * (len + 2 * EQ_PAD) + 2 * EQ_MAX_TAPS + (descent ? EQ_SUMS * FR_WAVES : 0);
}

// The frame into its two padded planes (a barrier must follow)
__device__ __forceinline__ void stage_padded(float* zr, float* zi, const float* src, int len, int planar, int tid) {
  for (int i = tid; i < len + 2 * EQ_PAD; i += FR_THREADS) {
    const int n = i - EQ_PAD;
    float2 v = make_float2(0.f, 0.f);
    if ((unsigned)n < (unsigned)len) v = load_sample(src, len, planar, n);
    zr[i] = v.x;
    zi[i] = v.y;
  }
}

template <int L>
__global__ __launch_bounds__(FR_THREADS) void frames_equalise_kernel(EqArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & (IQ_WAVE - 1), wave = tid >> 6;
  const int len = a.len, S = len + 2 * EQ_PAD;
  constexpr int c = L / 2;
  const long fi = blockIdx.x;
  const float* src = a.x + fi * 2 * len;
  float* dst = a.out + fi * 2 * len;
  float* zr = lds;
  float* zi = zr + S;
  float* wl = zi + S;                                      // w[l] at wl[2 l], wl[2 l + 1]
  float* red = wl + 2 * EQ_MAX_TAPS;                       // [EQ_SUMS][FR_WAVES]
  const float R = a.modulus, mu = a.mu, flen = (float)len;
  const bool cma = a.mode == IQ_EQ_CMA;
  const int T = cma ? a.iters : 0;

  stage_padded(zr, zi, src, len, a.planar, tid);
  if (tid < 2 * L) {
    const float* from = cma ? a.w0 : a.w;
    wl[tid] = from ? from[fi * 2 * L + tid] : (tid == 2 * c ? 1.f : 0.f);
  }
  __syncthreads();

  float j_first = nanf(""), j_last = 0.f;                  // thread 0's
  for (int t = 0;; ++t) {
    const bool last = t == T;
    float wr[L], wi[L], gr[L], gi[L];
#pragma unroll
    for (int l = 0; l < L; ++l) {
      wr[l] = wl[2 * l];
      wi[l] = wl[2 * l + 1];
      gr[l] = gi[l] = 0.f;
    }
    float js = 0.f;
#pragma unroll 1
    for (int n = tid; n < len; n += FR_THREADS) {
      const float* pr = zr + n + c + EQ_PAD;
      const float* pi = zi + n + c + EQ_PAD;
      float xr[L], xi[L];
      float yr = 0.f, yi = 0.f;
#pragma unroll
      for (int l = 0; l < L; ++l) {
        xr[l] = pr[-l];
        xi[l] = pi[-l];
        yr = fmaf(-xi[l], wi[l], fmaf(xr[l], wr[l], yr));
        yi = fmaf(xi[l], wr[l], fmaf(xr[l], wi[l], yi));
      }
      const float d = __fsub_rn(fmaf(yi, yi, __fmul_rn(yr, yr)), R);
      js = fmaf(d, d, js);
      if (last) {
        store_sample(dst, len, a.planar, n, make_float2(yr, yi));
      } else {
        const float er = __fmul_rn(yr, d), ei = __fmul_rn(yi, d);
#pragma unroll
        for (int l = 0; l < L; ++l) {
          gr[l] = fmaf(xi[l], ei, fmaf(xr[l], er, gr[l]));
          gi[l] = fmaf(-xi[l], er, fmaf(xr[l], ei, gi[l]));
        }
      }
    }
    js = wave_sum(js);
    if (lane == 0) red[2 * EQ_MAX_TAPS * FR_WAVES + wave] = js;
    if (!last) {
#pragma unroll
      for (int l = 0; l < L; ++l) {
        const float sr = wave_sum(gr[l]), si = wave_sum(gi[l]);
        if (lane == 0) { red[(2 * l) * FR_WAVES + wave] = sr; red[(2 * l + 1) * FR_WAVES + wave] = si; }
      }
    }
    __syncthreads();
    if (tid == 0) {
      j_last = __fdiv_rn(red_sum(red + 2 * EQ_MAX_TAPS * FR_WAVES), flen);
      if (t == 0 && cma) j_first = j_last;
    }
    if (last) break;
    if (tid < 2 * L) wl[tid] = fmaf(-mu, __fdiv_rn(red_sum(red + tid * FR_WAVES), flen), wl[tid]);
    __syncthreads();
  }
  // w is final: nothing has written it since the last barrier
  if (a.w_out && tid < 2 * L) a.w_out[fi * 2 * L + tid] = wl[tid];
  if (a.est && tid == 0) {
    float e2 = 0.f, best = 0.f;
    int at = 0;
    for (int l = 0; l < L; ++l) {
      const float re = wl[2 * l], im = wl[2 * l + 1];
      e2 = fmaf(im, im, fmaf(re, re, e2));
      const float m = fmaf(im, im, __fmul_rn(re, re));
      if (l == 0 || m > best) { best = m; at = l; }
    }
    a.est[4 * fi + 0] = j_first;
    a.est[4 * fi + 1] = j_last;
    a.est[4 * fi + 2] = e2;
    a.est[4 * fi + 3] = (float)at;
  }
}

// dx[m] = sum_l conj(w[l]) dout[m - c + l]
template <int L>
__global__ __launch_bounds__(FR_THREADS) void frames_equalise_bwd_kernel(EqArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x;
  const int len = a.len, S = len + 2 * EQ_PAD;
  constexpr int c = L / 2;
  const long fi = blockIdx.x;
  float* dst = a.out + fi * 2 * len;
  float* zr = lds;
  float* zi = zr + S;
  float* wl = zi + S;
  stage_padded(zr, zi, a.x + fi * 2 * len, len, a.planar, tid);
  if (tid < 2 * L) wl[tid] = a.w[fi * 2 * L + tid];
  __syncthreads();
  float wr[L], wi[L];
#pragma unroll
  for (int l = 0; l < L; ++l) {
    wr[l] = wl[2 * l];
    wi[l] = wl[2 * l + 1];
  }
#pragma unroll 1
  for (int m = tid; m < len; m += FR_THREADS) {
    const float* pr = zr + m - c + EQ_PAD;
    const float* pi = zi + m - c + EQ_PAD;
    float yr = 0.f, yi = 0.f;
#pragma unroll
    for (int l = 0; l < L; ++l) {
      const float dr = pr[l], di = pi[l];
      yr = fmaf(di, wi[l], fmaf(dr, wr[l], yr));
      yi = fmaf(-dr, wi[l], fmaf(di, wr[l], yi));
    }
    store_sample(dst, len, a.planar, m, make_float2(yr, yi));
  }
}

// -> IQ_OK or the refusal; nothing is launched and no pointer but par dereferenced before this returns IQ_OK.
// given: the weights come from par->w (IQ_EQ_GIVEN, the backward)
int check(const void* in, const void* out, int len, const iq_equaliser_t* p, bool given) {
  if (!in || !out || !p) return IQ_ERR_ARG;
  if (p->taps < 1 || len < 1 || p->iters < 0) return IQ_ERR_ARG;
  if (!is_finite(p->mu) || !is_finite(p->modulus) || p->mu < 0.f) return IQ_ERR_ARG;
  if ((p->planar & ~1) || (p->mode != IQ_EQ_GIVEN && p->mode != IQ_EQ_CMA)) return IQ_ERR_ARG;
  const uintptr_t io = p->planar ? 3 : 7;                  // interleaved frames move as (I, Q) pairs
  if (((uintptr_t)in & io) || ((uintptr_t)out & io)) return IQ_ERR_ARG;
  if (((uintptr_t)p->w & 3) || ((uintptr_t)p->w0 & 3)) return IQ_ERR_ARG;
  if (given && !p->w) return IQ_ERR_ARG;
  if (p->taps > EQ_MAX_TAPS || p->iters > EQ_MAX_ITERS || !frame_fits(len)) return IQ_ERR_UNSUPPORTED;
  return IQ_OK;
}

// The instance of the tap count a.taps (1 .. EQ_MAX_TAPS: check has seen to it)
template <int L = 1>
void launch_taps(bool bwd, int n_frames, size_t lds, hipStream_t st, const EqArgs& a) {
  if (a.taps == L) {
    if (bwd) launch_frames(frames_equalise_bwd_kernel<L>, n_frames, lds, st, a);
    else launch_frames(frames_equalise_kernel<L>, n_frames, lds, st, a);
  } else if constexpr (L < EQ_MAX_TAPS) {
    launch_taps<L + 1>(bwd, n_frames, lds, st, a);
  }
}

EqArgs pack(int len, const iq_equaliser_t* p) {
  EqArgs a = {};
  a.w = p->w; a.w0 = p->w0;
  a.len = len; a.taps = p->taps; a.iters = p->iters; a.planar = p->planar; a.mode = p->mode;
  a.mu = p->mu; a.modulus = p->modulus;
  return a;
}

}  // namespace

extern "C" int iq_frames_equalise(const float* x, float* out, float* w_out, float* est, int n_frames, int len,
                                  const iq_equaliser_t* par, iq_stream_t stream) {
  int rc = check(x, out, len, par, par && par->mode == IQ_EQ_GIVEN);
  if (rc == IQ_OK && (((uintptr_t)w_out & 3) || ((uintptr_t)est & 3))) rc = IQ_ERR_ARG;
  if (rc != IQ_OK) return rc;
  if (n_frames <= 0) return IQ_OK;
  hipStream_t st = (hipStream_t)stream;
  IQ_PROF(IQ_FAM_MISC, st);
  EqArgs a = pack(len, par);
  a.x = x; a.out = out; a.w_out = w_out; a.est = est;
  const double passes = par->mode == IQ_EQ_CMA ? par->iters : 0;
  IQ_PROF_K((double)n_frames * len * 16, (double)n_frames * len * par->taps * (8.0 + 16.0 * passes), "frames_equalise_kernel<%d>", par->taps);
  launch_taps(false, n_frames, eq_lds_floats(len, true) * sizeof(float), st, a);
  return iq_launch_status();
}

extern "C" int iq_frames_equalise_bwd(const float* dout, float* dx, int n_frames, int len, const iq_equaliser_t* par,
                                      iq_stream_t stream) {
  const int rc = check(dout, dx, len, par, true);
  if (rc != IQ_OK) return rc;
  if (n_frames <= 0) return IQ_OK;
  hipStream_t st = (hipStream_t)stream;
  IQ_PROF(IQ_FAM_MISC, st);
  EqArgs a = pack(len, par);
  a.x = dout; a.out = dx;
  IQ_PROF_K((double)n_frames * len * 16, (double)n_frames * len * par->taps * 8.0, "frames_equalise_bwd_kernel<%d>", par->taps);
  launch_taps(true, n_frames, eq_lds_floats(len, false) * sizeof(float), st, a);
  return iq_launch_status();
}
