// Tracking equaliser (iq_frames_equalise_track / _bwd, include/iqvit.h): block constant-modulus descent per overlapping segment
// of a frame, and a filter whose weights are interpolated between the segments' centres.  Three kernels, plain VALU.
//
// 1. track_descent_kernel<L>: one WAVE per (frame, segment), four per workgroup; wave g = 4 blockIdx.x + wave is segment g % S of
//    frame g / S, so a frame's segments are neighbours in the grid and share its lines of L2.  The wave stages the seg + L - 1
//    samples its segment's windows reach (zeros outside the frame) and the taper into its own slice of LDS; one barrier; then all
//    `iters` steps run without another: lane k % 64 owns outputs k, k + 64, .. (at most 8), takes each window from the slice into
//    registers, runs the fmaf chain of y, forms e and adds conj(window) e to its 2 L gradient sums; the butterflies leave every
//    sum in every lane, so every lane steps its own copy of w: the weights and the sums never leave the registers (a template on
//    L as in equaliser.hip: 6 L registers, no scratch).  Lanes read consecutive words of a plane: no bank conflict.
// 2. track_filter_kernel: one workgroup per frame.  The frame as two padded planes (as equaliser.hip), the S x L weights, w0 and
//    the sums in LDS; thread n % 256 owns output n, forms w(n)[l] from the two neighbouring segments' words as it goes down the
//    chain (lanes of a wave mostly share j: LDS broadcasts) and adds d^2 to its J.  A second pass under w0 alone gives est[0] when
//    est is asked for under CMA.  The same kernel serves GIVEN (and then copies w to w_out).
// 3. track_bwd_kernel: the filter's shape, gathering: dx[m] = sum_l conj(w(m - c + l)[l]) dout[m - c + l].
//
// Indices.  Slice (descent): sample p of the slice is frame sample j hop - (L - 1 - c) + p, p < seg + L - 1 <= 543 < TR_SLICE; the
// window of output k reads p = k + L - 1 - l, l < L: from k >= 0 to k + L - 1 <= seg + L - 2.  Planes (filter, adjoint): as in
// equaliser.hip, n + c - l + TR_PAD and m - c + l + TR_PAD stay 16 words inside the padded plane.  Weights in LDS: (j L + l) 2 with
// j <= S - 1 (segment_of clamps both ends, for any integer n).  Memory: frame fi at x + fi 2 len (long); w, w_out at
// ((fi S + j) L + l) 2; w0 at (fi L + l) 2; est at 4 fi; taper at k < seg.
#include <math.h>

#include "frames.h"
#include "iqvit.h"
#include "prof.h"

namespace {

constexpr int TR_MAX_TAPS = 32, TR_MAX_ITERS = 4096, TR_MAX_SEG = 512, TR_MAX_SEGMENTS = 256, TR_PAD = 32;
constexpr int TR_SLICE = 544;                              // >= TR_MAX_SEG + TR_MAX_TAPS - 1 samples per plane of a wave's slice
constexpr int TR_SLICE_FLOATS = 2 * TR_SLICE + TR_MAX_SEG; // zr | zi | taper

struct TrArgs {
  const float* x;       // forward: the frames; backward: dout
  float* out;           // forward: out; backward: dx
  const float* w;       // the segments' weights the filter reads: [n,S,L,2]
  const float* w0;
  const float* taper;
  float* w_out;
  float* est;
  int n_frames, len, taps, iters, planar, cma, seg, hop, S;
  float mu, modulus;
};

__host__ __device__ inline size_t tr_filter_floats(int len, int taps, int S) {
  return (size_t)2 * (len + 2 * TR_PAD) + (size_t)2 * taps * S + 2 * TR_MAX_TAPS + FR_WAVES + TR_MAX_SEGMENTS;
}

// The frame into its two padded planes (a barrier must follow)
__device__ __forceinline__ void stage_planes(float* zr, float* zi, const float* src, int len, int planar, int tid) {
  for (int i = tid; i < len + 2 * TR_PAD; i += FR_THREADS) {
    const int n = i - TR_PAD;
    float2 v = make_float2(0.f, 0.f);
    if ((unsigned)n < (unsigned)len) v = load_sample(src, len, planar, n);
    zr[i] = v.x;
    zi[i] = v.y;
  }
}

// Output n (any integer) -> the segment j whose weights it starts from and the share a of the next one's; edge: w(n) = w_j itself
struct SegAt {
  int j;
  float a;
  bool edge;
};
__device__ __forceinline__ SegAt segment_of(int n, int seg, int hop, int S) {
  const int t = n - seg / 2;
  if (t <= 0) return SegAt{0, 0.f, true};
  if (t >= (S - 1) * hop) return SegAt{S - 1, 0.f, true};
  return SegAt{t / hop, __fdiv_rn((float)(t % hop), (float)hop), false};
}
// One word of w(n): wa the word of segment j, wb of segment j + 1
__device__ __forceinline__ float word_at(float wa, float wb, SegAt s) { return s.edge ? wa : fmaf(s.a, __fsub_rn(wb, wa), wa); }

template <int L>
__global__ __launch_bounds__(FR_THREADS) void track_descent_kernel(TrArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & (IQ_WAVE - 1), wave = tid >> 6;
  constexpr int c = L / 2;
  const int len = a.len, seg = a.seg, S = a.S;
  const long g = (long)blockIdx.x * FR_WAVES + wave;
  const bool active = g < (long)a.n_frames * S;            // the last workgroup's spare waves only keep the barrier company
  const long fi = active ? g / S : 0;
  const int j = active ? (int)(g % S) : 0;
  float* zr = lds + wave * TR_SLICE_FLOATS;
  float* zi = zr + TR_SLICE;
  float* h = zi + TR_SLICE;
  float wr[L], wi[L];
  if (active) {
    const float* src = a.x + fi * 2 * len;
    const int first = j * a.hop - (L - 1 - c);
    for (int p = lane; p < seg + L - 1; p += IQ_WAVE) {
      const int n = first + p;
      float2 v = make_float2(0.f, 0.f);
      if ((unsigned)n < (unsigned)len) v = load_sample(src, len, a.planar, n);
      zr[p] = v.x;
      zi[p] = v.y;
    }
    for (int k = lane; k < seg; k += IQ_WAVE) h[k] = a.taper[k];
#pragma unroll
    for (int l = 0; l < L; ++l) {
      wr[l] = a.w0 ? a.w0[(fi * L + l) * 2] : (l == c ? 1.f : 0.f);
      wi[l] = a.w0 ? a.w0[(fi * L + l) * 2 + 1] : 0.f;
    }
  }
  __syncthreads();
  if (!active) return;
  const float R = a.modulus, mu = a.mu;
#pragma unroll 1
  for (int t = 0; t < a.iters; ++t) {
    float gr[L], gi[L];
#pragma unroll
    for (int l = 0; l < L; ++l) gr[l] = gi[l] = 0.f;
#pragma unroll 1
    for (int k = lane; k < seg; k += IQ_WAVE) {
      const float* pr = zr + k + L - 1;
      const float* pi = zi + k + L - 1;
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
      const float hk = h[k];
      const float er = __fmul_rn(__fmul_rn(yr, d), hk), ei = __fmul_rn(__fmul_rn(yi, d), hk);
#pragma unroll
      for (int l = 0; l < L; ++l) {
        gr[l] = fmaf(xi[l], ei, fmaf(xr[l], er, gr[l]));
        gi[l] = fmaf(-xi[l], er, fmaf(xr[l], ei, gi[l]));
      }
    }
#pragma unroll
    for (int l = 0; l < L; ++l) {                          // the butterfly leaves the sum in every lane: every lane steps its copy
      wr[l] = fmaf(-mu, wave_sum(gr[l]), wr[l]);
      wi[l] = fmaf(-mu, wave_sum(gi[l]), wi[l]);
    }
  }
  if (lane == 0) {
    float* dst = a.w_out + (fi * S + j) * 2 * L;
#pragma unroll
    for (int l = 0; l < L; ++l) {
      dst[2 * l] = wr[l];
      dst[2 * l + 1] = wi[l];
    }
  }
}

// LDS of the filter and the adjoint: zr [P] | zi [P] | ws [S][L][2] | w0 [2 TR_MAX_TAPS] | red [FR_WAVES] | dj [TR_MAX_SEGMENTS], P = len + 2 TR_PAD
__global__ __launch_bounds__(FR_THREADS) void track_filter_kernel(TrArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & (IQ_WAVE - 1), wave = tid >> 6;
  const int len = a.len, P = len + 2 * TR_PAD, L = a.taps, c = L / 2, S = a.S, seg = a.seg, hop = a.hop;
  const long fi = blockIdx.x;
  const float* src = a.x + fi * 2 * len;
  float* dst = a.out + fi * 2 * len;
  float* zr = lds;
  float* zi = zr + P;
  float* ws = zi + P;
  float* w0 = ws + 2 * L * S;
  float* red = w0 + 2 * TR_MAX_TAPS;
  float* dj = red + FR_WAVES;
  const float R = a.modulus, flen = (float)len;
  const bool cma = a.cma != 0;

  stage_planes(zr, zi, src, len, a.planar, tid);
  const float* wsrc = a.w + fi * 2 * L * S;
  for (int i = tid; i < 2 * L * S; i += FR_THREADS) {
    const float v = wsrc[i];
    ws[i] = v;
    if (!cma && a.w_out) a.w_out[fi * 2 * L * S + i] = v;  // GIVEN: w_out is a copy of w (under CMA the descent wrote it)
  }
  if (cma && tid < 2 * L) w0[tid] = a.w0 ? a.w0[fi * 2 * L + tid] : (tid == 2 * c ? 1.f : 0.f);
  __syncthreads();

  // pass 0: out and J(out) under w(n); pass 1 (est under CMA only): J under w0 alone
  const int passes = (a.est && cma) ? 2 : 1;
  float j_out = 0.f, j_w0 = nanf("");                      // thread 0's
  for (int pass = 0; pass < passes; ++pass) {
    float js = 0.f;
#pragma unroll 1
    for (int n = tid; n < len; n += FR_THREADS) {
      const float* pr = zr + n + c + TR_PAD;
      const float* pi = zi + n + c + TR_PAD;
      const SegAt s = pass == 0 ? segment_of(n, seg, hop, S) : SegAt{0, 0.f, true};
      const float* wa = pass == 0 ? ws + (size_t)s.j * 2 * L : w0;
      const float* wb = s.edge ? wa : wa + 2 * L;
      float yr = 0.f, yi = 0.f;
#pragma unroll 4
      for (int l = 0; l < L; ++l) {
        const float xr = pr[-l], xi = pi[-l];
        const float wr = word_at(wa[2 * l], wb[2 * l], s), wi = word_at(wa[2 * l + 1], wb[2 * l + 1], s);
        yr = fmaf(-xi, wi, fmaf(xr, wr, yr));
        yi = fmaf(xi, wr, fmaf(xr, wi, yi));
      }
      const float d = __fsub_rn(fmaf(yi, yi, __fmul_rn(yr, yr)), R);
      js = fmaf(d, d, js);
      if (pass == 0) store_sample(dst, len, a.planar, n, make_float2(yr, yi));
    }
    js = wave_sum(js);
    __syncthreads();                                       // (the second pass: red has been read)
    if (lane == 0) red[wave] = js;
    __syncthreads();
    if (tid == 0) {
      const float J = __fdiv_rn(red_sum(red), flen);
      if (pass == 0) j_out = J; else j_w0 = J;
    }
  }
  if (!a.est) return;
  // how far the weights moved: D_j by thread j, the maximum by thread 0
  if (cma && tid < S) {
    const float* wj = ws + (size_t)tid * 2 * L;
    float acc = 0.f;
    for (int l = 0; l < L; ++l) {
      const float dr = __fsub_rn(wj[2 * l], w0[2 * l]), di = __fsub_rn(wj[2 * l + 1], w0[2 * l + 1]);
      acc = fmaf(di, di, fmaf(dr, dr, acc));
    }
    dj[tid] = acc;
  }
  __syncthreads();
  if (tid == 0) {
    float best = nanf("");
    if (cma) {
      best = dj[0];
      for (int j = 1; j < S; ++j)
        if (dj[j] > best) best = dj[j];
    }
    a.est[4 * fi + 0] = j_w0;
    a.est[4 * fi + 1] = j_out;
    a.est[4 * fi + 2] = best;
    a.est[4 * fi + 3] = (float)S;
  }
}

// dx[m] = sum_l conj(w(n)[l]) dout[n], n = m - c + l
__global__ __launch_bounds__(FR_THREADS) void track_bwd_kernel(TrArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x;
  const int len = a.len, P = len + 2 * TR_PAD, L = a.taps, c = L / 2, S = a.S, seg = a.seg, hop = a.hop;
  const long fi = blockIdx.x;
  float* dst = a.out + fi * 2 * len;
  float* zr = lds;
  float* zi = zr + P;
  float* ws = zi + P;
  stage_planes(zr, zi, a.x + fi * 2 * len, len, a.planar, tid);
  const float* wsrc = a.w + fi * 2 * L * S;
  for (int i = tid; i < 2 * L * S; i += FR_THREADS) ws[i] = wsrc[i];
  __syncthreads();
#pragma unroll 1
  for (int m = tid; m < len; m += FR_THREADS) {
    const float* pr = zr + m - c + TR_PAD;
    const float* pi = zi + m - c + TR_PAD;
    float yr = 0.f, yi = 0.f;
#pragma unroll 4
    for (int l = 0; l < L; ++l) {
      const SegAt s = segment_of(m - c + l, seg, hop, S);
      const float* wa = ws + (size_t)s.j * 2 * L;
      const float* wb = s.edge ? wa : wa + 2 * L;
      const float wr = word_at(wa[2 * l], wb[2 * l], s), wi = word_at(wa[2 * l + 1], wb[2 * l + 1], s);
      const float dr = pr[l], di = pi[l];
      yr = fmaf(di, wi, fmaf(dr, wr, yr));
      yi = fmaf(-dr, wi, fmaf(di, wr, yi));
    }
    store_sample(dst, len, a.planar, m, make_float2(yr, yi));
  }
}

// -> IQ_OK or the refusal; nothing is launched and no pointer but p dereferenced before this returns IQ_OK.
// given: the weights come from p->w (IQ_EQT_GIVEN, the backward); fwd: the forward, whose CMA needs the taper
int check(const void* in, const void* out, int len, const iq_equaliser_track_t* p, bool given, bool fwd) {
  if (!in || !out || !p) return IQ_ERR_ARG;
  if (p->taps < 1 || len < 1 || p->iters < 0 || p->seg < 1 || p->hop < 1 || p->hop > p->seg || len < p->seg) return IQ_ERR_ARG;
  if (!is_finite(p->mu) || !is_finite(p->modulus) || p->mu < 0.f) return IQ_ERR_ARG;
  if ((p->planar & ~1) || (p->mode != IQ_EQT_GIVEN && p->mode != IQ_EQT_CMA)) return IQ_ERR_ARG;
  const uintptr_t io = p->planar ? 3 : 7;                  // interleaved frames move as (I, Q) pairs
  if (((uintptr_t)in & io) || ((uintptr_t)out & io)) return IQ_ERR_ARG;
  if (((uintptr_t)p->w & 3) || ((uintptr_t)p->w0 & 3) || ((uintptr_t)p->taper & 3)) return IQ_ERR_ARG;
  if (given && !p->w) return IQ_ERR_ARG;
  if (fwd && !given && !p->taper) return IQ_ERR_ARG;
  if (p->taps > TR_MAX_TAPS || p->iters > TR_MAX_ITERS || p->seg > TR_MAX_SEG || !frame_fits(len)) return IQ_ERR_UNSUPPORTED;
  if ((len - p->seg) / p->hop + 1 > TR_MAX_SEGMENTS) return IQ_ERR_UNSUPPORTED;
  return IQ_OK;
}

// The descent's instance of the tap count a.taps (1 .. TR_MAX_TAPS: check has seen to it)
template <int L = 1>
void launch_descent(dim3 grid, hipStream_t st, const TrArgs& a) {
  if (a.taps == L) {
    launch_frames(track_descent_kernel<L>, grid, FR_WAVES * TR_SLICE_FLOATS * sizeof(float), st, a);
  } else if constexpr (L < TR_MAX_TAPS) {
    launch_descent<L + 1>(grid, st, a);
  }
}

TrArgs pack(int n_frames, int len, const iq_equaliser_track_t* p) {
  TrArgs a = {};
  a.w = p->w; a.w0 = p->w0; a.taper = p->taper;
  a.n_frames = n_frames; a.len = len; a.taps = p->taps; a.iters = p->iters; a.planar = p->planar;
  a.cma = p->mode == IQ_EQT_CMA; a.seg = p->seg; a.hop = p->hop; a.S = (len - p->seg) / p->hop + 1;
  a.mu = p->mu; a.modulus = p->modulus;
  return a;
}

}  // namespace

extern "C" int iq_frames_equalise_track(const float* x, float* out, float* w_out, float* est, int n_frames, int len,
                                        const iq_equaliser_track_t* par, iq_stream_t stream) {
  const bool given = par && par->mode == IQ_EQT_GIVEN;
  int rc = check(x, out, len, par, given, true);
  if (rc == IQ_OK && (((uintptr_t)w_out & 3) || ((uintptr_t)est & 3) || (!given && !w_out))) rc = IQ_ERR_ARG;
  if (rc != IQ_OK) return rc;
  if (n_frames <= 0) return IQ_OK;
  hipStream_t st = (hipStream_t)stream;
  TrArgs a = pack(n_frames, len, par);
  a.x = x; a.out = out; a.w_out = w_out; a.est = est;
  const double outputs = (double)n_frames * len, taps = par->taps;
  if (!given) {
    IQ_PROF(IQ_FAM_MISC, st);
    const double waves = (double)n_frames * a.S;
    IQ_PROF_K(waves * ((par->seg + taps - 1) * 8.0 + taps * 8.0), waves * par->seg * taps * 16.0 * par->iters, "track_descent_kernel<%d>",
              par->taps);
    launch_descent(dim3((unsigned)(((long)n_frames * a.S + FR_WAVES - 1) / FR_WAVES)), st, a);
    a.w = w_out;                                           // what the descent wrote is what the filter reads
  }
  {
    IQ_PROF(IQ_FAM_MISC, st);
    IQ_PROF_K(outputs * 16 + (double)n_frames * a.S * taps * 8, outputs * taps * 12.0 * ((est && !given) ? 2 : 1), "track_filter_kernel");
    launch_frames(track_filter_kernel, dim3((unsigned)n_frames), tr_filter_floats(len, par->taps, a.S) * sizeof(float), st, a);
  }
  return iq_launch_status();
}

extern "C" int iq_frames_equalise_track_bwd(const float* dout, float* dx, int n_frames, int len, const iq_equaliser_track_t* par,
                                            iq_stream_t stream) {
  const int rc = check(dout, dx, len, par, true, false);
  if (rc != IQ_OK) return rc;
  if (n_frames <= 0) return IQ_OK;
  hipStream_t st = (hipStream_t)stream;
  IQ_PROF(IQ_FAM_MISC, st);
  TrArgs a = pack(n_frames, len, par);
  a.x = dout; a.out = dx;
  IQ_PROF_K((double)n_frames * len * 16 + (double)n_frames * a.S * par->taps * 8, (double)n_frames * len * par->taps * 12.0, "track_bwd_kernel");
  launch_frames(track_bwd_kernel, dim3((unsigned)n_frames), tr_filter_floats(len, par->taps, a.S) * sizeof(float), st, a);
  return iq_launch_status();
}
