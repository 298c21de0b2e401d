// Carrier recovery (iq_frames_carrier / _bwd, include/iqvit.h): a blind frequency and phase estimate per frame from the line of
// the M-th power, and the derotation.  One workgroup per frame (workgroup size, launch and the fixed-order sum of the wave
// sums: frames.h).
//
// The periodogram of w = z^M over N = n1 * n2 points is a two-stage (Cooley-Tukey) pair of small DFT GEMMs on the fp32-input
// MFMA v_mfma_f32_32x32x2_f32, both through channel_step (frames.h), from tables that are plain numbers to the kernel:
//   stage 1   D[row = k1][col = b] = sum_a t1[a][k1] w[a n2 + b]       the table is the A operand, w in LDS the B operand
//   twiddle   Bm[k1, b] = D * (twc - j tws)[b k1], in the epilogue (rotate), into LDS
//   stage 2   D[row = k2][col = k1] = sum_b t2[b][k2] Bm[k1, b]        again table x LDS; the accumulator has k1 on the lane, so
//             P[k1 + n1 k2] is written 32 consecutive floats at a time
// A wave owns whole 32 x 32 tiles (tile = wave, wave + 4, ...); at most N / 1024 <= 8 tiles per stage.  The table operands come
// straight from memory: a half-wave reads 32 consecutive floats of one table row, at most 512 KB per table, which stay in L2.
//
// LDS: w planar [2][N] | Bm planar [2][n2][n1 + 1] | red [12] | peak [8] | box [4].  P [N] takes the place of w's real plane
// once stage 1 is done (a barrier in between), which is why the phase sum recomputes w from memory.  Bank conflicts (ds b32:
// bank = word % 32 within a half-wave): stage 1 reads w[a n2 + b] over consecutive b; its epilogue writes Bm for ONE k1 and 32
// different b per register, which at row stride n1 (a multiple of 32) would be 32 words on one bank: the stride n1 + 1 spreads
// them over all 32; stage 2 reads Bm[b (n1 + 1) + k1] over consecutive k1.  All three are conflict-free.  Bytes:
// 4 * (2 N + 2 n2 (n1 + 1) + 24) <= 128.3 KB of 160 KB at N = 8192.
//
// LDS indices.  w: a n2 + b < n1 n2 = N.  Bm: b (n1 + 1) + k1 <= (n2 - 1)(n1 + 1) + n1 - 1 < n2 (n1 + 1).  P: k1 + n1 k2 < N;
// the search reads s mod N and the refinement (k^ +- 1) mod N.  tw: b k1 <= (n2 - 1)(n1 - 1) < N.
//
// After the barrier behind P: the workgroup finds the peak (thread i % 256 the signed bins -k_max + i, then a butterfly and the
// four waves in order, under the total order "larger P, then lower s": the result is THE first maximum whatever the partition),
// thread 0 refines it and fixes F, the workgroup sums S = sum_n w[n] conj e(G n) (thread n % 256, n ascending, the butterfly,
// the four waves in order), thread 0 fixes TH and est, and every thread derotates its samples from memory.
#include <math.h>

#include "frames.h"
#include "iqvit.h"
#include "prof.h"

namespace {

constexpr int CR_MAX_N = 8192;

struct CrArgs {
  const float* x;       // forward: the frames; backward: dout
  float* out;           // forward: out; backward: dx
  float* est;
  int32_t* fth_out;
  float* power;
  const float* t1;
  const float* t2;
  const float* tw;
  const int32_t* fth;
  int len, order, n1, n2, N, k_max, refine, planar, mode;
  int s1;               // row stride of Bm: n1 + 1
};

// z^M by log2 M squarings, each a rotate() of the value by itself
__device__ __forceinline__ float2 mth_power(float2 z, int order) {
  for (int m = 1; m < order; m <<= 1) z = rotate(z, z.x, z.y);
  return z;
}

// e(p) = (cos, sin) of the integer phase p, units of 2^-32 turn
__device__ __forceinline__ void phase_cs(uint32_t p, float& c, float& s) { sincospif((float)(int32_t)p * 0x1p-31f, &s, &c); }

// the search key of a power: a NaN counts as +infinity
__device__ __forceinline__ float peak_key(float p) { return p == p ? p : INFINITY; }
// (k1, s1) comes before (k0, s0): larger key, then lower signed bin
__device__ __forceinline__ bool peak_before(float k1, int s1, float k0, int s0) { return k1 > k0 || (k1 == k0 && s1 < s0); }

// One 32 x 32 tile of a DFT stage: rows = the 32 table columns from tcol0, columns = the 32 LDS words from j0 (+ jstep per
// step of the sum), `depth` steps of the sum, two per channel_step.
__device__ __forceinline__ void dft_tile(f32x16& re, f32x16& im, const float* tc, const float* ts, int tn, int tcol0,
                                         const float* fI, const float* fQ, int j0, int jstep, int jlimit, int depth, int col,
                                         int half) {
  const float* pc = tc + (size_t)half * tn + tcol0 + col;
  const float* ps = ts + (size_t)half * tn + tcol0 + col;
  int j = j0 + half * jstep + col;
  float ac = pc[0], as = ps[0];
  for (int m = 0; m < depth; m += 2) {
    // the table entries of step m + 2 are requested before the MFMAs of step m (the last step asks for its own again)
    const size_t nx = m + 2 < depth ? (size_t)2 * tn : 0;
    pc += nx; ps += nx;
    const float nc = pc[0], ns = ps[0];
    channel_step(re, im, ac, as, fI, fQ, j, jlimit);
    ac = nc; as = ns;
    j += 2 * jstep;
  }
}

__global__ __launch_bounds__(FR_THREADS) void frames_carrier_kernel(CrArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & (IQ_WAVE - 1), wave = tid >> 6;
  const int col = lane & 31, half = lane >> 5;
  const int len = a.len, N = a.N, n1 = a.n1, n2 = a.n2, S1 = a.s1, M = a.order;
  const long fi = blockIdx.x;
  const float* src = a.x + fi * 2 * len;
  float* dst = a.out + fi * 2 * len;
  float* wr = lds;
  float* wi = wr + N;
  float* br = wi + N;
  float* bi = br + n2 * S1;
  float* red = bi + n2 * S1;                               // [3][FR_WAVES]
  float* pkey = red + 3 * FR_WAVES;                        // [FR_WAVES]
  int* pbin = reinterpret_cast<int*>(pkey + FR_WAVES);     // [FR_WAVES]
  int* box = pbin + FR_WAVES;                              // F, TH, valid

  uint32_t F = 0, TH = 0;
  if (a.mode == IQ_CR_ESTIMATE) {
    // ---- 1. w = z^M, zero behind the frame
    for (int n = tid; n < N; n += FR_THREADS) {
      float2 w = make_float2(0.f, 0.f);
      if (n < len) w = mth_power(load_sample(src, len, a.planar, n), M);
      wr[n] = w.x;
      wi[n] = w.y;
    }
    __syncthreads();
    // ---- 2. stage 1 and the twiddle: Bm[k1, b] at b * S1 + k1
    const int tb = n2 / FR_TILE, tiles1 = (n1 / FR_TILE) * tb;
    for (int t = wave; t < tiles1; t += FR_WAVES) {
      const int k10 = FR_TILE * (t / tb), b0 = FR_TILE * (t % tb);
      f32x16 re = {}, im = {};
      dft_tile(re, im, a.t1, a.t1 + (size_t)n1 * n1, n1, k10, wr, wi, b0, n2, N, n1, col, half);
      const int b = b0 + col;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int k1 = k10 + acc_row(r, half);
        const int i = b * k1;
        const float2 v = rotate(make_float2(re[r], im[r]), a.tw[i], -a.tw[N + i]);
        br[b * S1 + k1] = v.x;
        bi[b * S1 + k1] = v.y;
      }
    }
    __syncthreads();                                       // w has been read by every wave: P may take its place
    // ---- 3. stage 2 and the power: P[k1 + n1 k2]
    float* P = wr;
    const int tk = n1 / FR_TILE, tiles2 = (n2 / FR_TILE) * tk;
    for (int t = wave; t < tiles2; t += FR_WAVES) {
      const int k20 = FR_TILE * (t / tk), k10 = FR_TILE * (t % tk);
      f32x16 re = {}, im = {};
      dft_tile(re, im, a.t2, a.t2 + (size_t)n2 * n2, n2, k20, br, bi, k10, S1, n2 * S1, n2, col, half);
#pragma unroll
      for (int r = 0; r < 16; ++r) P[k10 + col + n1 * (k20 + acc_row(r, half))] = fmaf(im[r], im[r], re[r] * re[r]);
    }
    __syncthreads();
    if (a.power)
      for (int k = tid; k < N; k += FR_THREADS) a.power[fi * N + k] = P[k];
    // ---- 4. the first maximum over the signed bins
    const int hi = a.k_max < N / 2 - 1 ? a.k_max : N / 2 - 1;
    float bk = -1.f;
    int bs = 0x7fffffff;
    for (int s = tid - a.k_max; s <= hi; s += FR_THREADS) {
      const float k = peak_key(P[s < 0 ? s + N : s]);
      if (peak_before(k, s, bk, bs)) { bk = k; bs = s; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ok = __shfl_xor(bk, o, IQ_WAVE);
      const int os = __shfl_xor(bs, o, IQ_WAVE);
      if (peak_before(ok, os, bk, bs)) { bk = ok; bs = os; }
    }
    if (lane == 0) { pkey[wave] = bk; pbin[wave] = bs; }
    __syncthreads();
    // ---- 5, 6. refinement and frequency: one thread
    if (tid == 0) {
      for (int w = 1; w < FR_WAVES; ++w)
        if (peak_before(pkey[w], pbin[w], bk, bs)) { bk = pkey[w]; bs = pbin[w]; }
      const int kh = bs < 0 ? bs + N : bs;
      const float pb = P[kh];
      const bool valid = pb != 0.f && fabsf(pb) < INFINITY;
      float d = 0.f;
      if (valid && a.refine) {
        const float pa = P[kh == 0 ? N - 1 : kh - 1], pc = P[kh == N - 1 ? 0 : kh + 1];
        const float den = __fadd_rn(__fsub_rn(pa, __fadd_rn(pb, pb)), pc);
        if (den < 0.f && fabsf(den) < INFINITY) d = fminf(fmaxf(__fdiv_rn(__fmul_rn(0.5f, __fsub_rn(pa, pc)), den), -0.5f), 0.5f);
      }
      uint32_t f = 0;
      if (valid) f = (uint32_t)llrint(((double)bs + (double)d) / ((double)N * (double)M) * 4294967296.0);
      box[0] = (int)f;
      box[1] = 0;
      box[2] = valid ? 1 : 0;
      if (a.est) {
        a.est[4 * fi + 0] = (float)((double)(int32_t)f * 0x1p-32);
        a.est[4 * fi + 2] = (float)bs + d;
        if (!valid) a.est[4 * fi + 1] = a.est[4 * fi + 3] = 0.f;
      }
    }
    __syncthreads();
    F = (uint32_t)box[0];
    if (box[2]) {                                          // workgroup-uniform
      // ---- 7. phase: S = sum_n w[n] conj e(G n), w recomputed from memory
      const uint32_t G = F * (uint32_t)M;
      float sr = 0.f, si = 0.f, pw = 0.f;
      for (int n = tid; n < len; n += FR_THREADS) {
        const float2 w = mth_power(load_sample(src, len, a.planar, n), M);
        float c, s;
        phase_cs(G * (uint32_t)n, c, s);
        const float2 v = rotate(w, c, -s);
        sr += v.x;
        si += v.y;
        pw = fmaf(w.y, w.y, fmaf(w.x, w.x, pw));
      }
      sr = wave_sum(sr); si = wave_sum(si); pw = wave_sum(pw);
      if (lane == 0) { red[wave] = sr; red[FR_WAVES + wave] = si; red[2 * FR_WAVES + wave] = pw; }
      __syncthreads();
      if (tid == 0) {
        const float Sr = red_sum(red), Si = red_sum(red + FR_WAVES), Pw = red_sum(red + 2 * FR_WAVES);
        const uint32_t th = (uint32_t)llrint(atan2((double)Si, (double)Sr) / (6.283185307179586476925 * (double)M) * 4294967296.0);
        box[1] = (int)th;
        if (a.est) {
          a.est[4 * fi + 1] = (float)((double)(int32_t)th * 0x1p-32 * 6.283185307179586476925);
          const float den = __fmul_rn((float)len, Pw);
          a.est[4 * fi + 3] = den > 0.f ? __fdiv_rn(fmaf(Si, Si, __fmul_rn(Sr, Sr)), den) : 0.f;
        }
      }
      __syncthreads();
    }
    TH = (uint32_t)box[1];
    if (tid == 0 && a.fth_out) {
      a.fth_out[2 * fi + 0] = (int32_t)F;
      a.fth_out[2 * fi + 1] = (int32_t)TH;
    }
  } else {
    F = (uint32_t)a.fth[2 * fi + 0];
    TH = (uint32_t)a.fth[2 * fi + 1];
    if (tid == 0) {
      if (a.fth_out) {
        a.fth_out[2 * fi + 0] = (int32_t)F;
        a.fth_out[2 * fi + 1] = (int32_t)TH;
      }
      if (a.est) {
        a.est[4 * fi + 0] = (float)((double)(int32_t)F * 0x1p-32);
        a.est[4 * fi + 1] = (float)((double)(int32_t)TH * 0x1p-32 * 6.283185307179586476925);
        a.est[4 * fi + 2] = a.est[4 * fi + 3] = nanf("");
      }
    }
  }
  // ---- 8. out[n] = z[n] conj e(F n + TH)
  for (int n = tid; n < len; n += FR_THREADS) {
    float c, s;
    phase_cs(F * (uint32_t)n + TH, c, s);
    store_sample(dst, len, a.planar, n, rotate(load_sample(src, len, a.planar, n), c, -s));
  }
}

// dx[n] = dout[n] e(F n + TH)
__global__ __launch_bounds__(FR_THREADS) void frames_carrier_bwd_kernel(CrArgs a) {
  const int tid = threadIdx.x, len = a.len;
  const long fi = blockIdx.x;
  const float* src = a.x + fi * 2 * len;
  float* dst = a.out + fi * 2 * len;
  const uint32_t F = (uint32_t)a.fth[2 * fi + 0], TH = (uint32_t)a.fth[2 * fi + 1];
  for (int n = tid; n < len; n += FR_THREADS) {
    float c, s;
    phase_cs(F * (uint32_t)n + TH, c, s);
    store_sample(dst, len, a.planar, n, rotate(load_sample(src, len, a.planar, n), c, s));
  }
}

// -> IQ_OK or the refusal; nothing is launched and no pointer but par dereferenced before this returns IQ_OK.
// given: the frequency and phase come from par->fth and no table is read (IQ_CR_GIVEN, the backward)
int check(const void* in, const void* out, int len, const iq_carrier_t* p, bool given) {
  if (!in || !out || !p) return IQ_ERR_ARG;
  if (p->order != 1 && p->order != 2 && p->order != 4 && p->order != 8) return IQ_ERR_ARG;
  if ((p->refine & ~1) || (p->planar & ~1) || (p->mode != IQ_CR_GIVEN && p->mode != IQ_CR_ESTIMATE) || len < 1) return IQ_ERR_ARG;
  const long N = (long)p->n1 * (long)p->n2;
  if (p->k_max < 0 || (long)p->k_max > N / 2) return IQ_ERR_ARG;
  const uintptr_t io = p->planar ? 3 : 7;                  // interleaved frames move as (I, Q) pairs
  if (((uintptr_t)in & io) || ((uintptr_t)out & io)) return IQ_ERR_ARG;
  if (((uintptr_t)p->t1 & 3) || ((uintptr_t)p->t2 & 3) || ((uintptr_t)p->tw & 3) || ((uintptr_t)p->fth & 3)) return IQ_ERR_ARG;
  if (given ? !p->fth : (!p->t1 || !p->t2 || !p->tw)) return IQ_ERR_ARG;
  if (!fft_size_ok(p->n1) || !fft_size_ok(p->n2) || N < len || N > CR_MAX_N || !frame_fits(len)) return IQ_ERR_UNSUPPORTED;
  return IQ_OK;
}

CrArgs pack(int len, const iq_carrier_t* p) {
  CrArgs a = {};
  a.t1 = p->t1; a.t2 = p->t2; a.tw = p->tw; a.fth = p->fth;
  a.len = len; a.order = p->order; a.n1 = p->n1; a.n2 = p->n2; a.N = p->n1 * p->n2; a.k_max = p->k_max;
  a.refine = p->refine; a.planar = p->planar; a.mode = p->mode;
  a.s1 = p->n1 + 1;
  return a;
}

}  // namespace

extern "C" int iq_frames_carrier(const float* x, float* out, float* est, int32_t* fth_out, float* power, int n_frames, int len,
                                 const iq_carrier_t* par, iq_stream_t stream) {
  int rc = check(x, out, len, par, par && par->mode == IQ_CR_GIVEN);
  if (rc == IQ_OK && (((uintptr_t)est & 3) || ((uintptr_t)fth_out & 3) || ((uintptr_t)power & 3))) rc = IQ_ERR_ARG;
  if (rc == IQ_OK && par->mode == IQ_CR_GIVEN && power) rc = IQ_ERR_ARG;
  if (rc != IQ_OK) return rc;
  if (n_frames <= 0) return IQ_OK;
  hipStream_t st = (hipStream_t)stream;
  IQ_PROF(IQ_FAM_MISC, st);
  CrArgs a = pack(len, par);
  a.x = x; a.out = out; a.est = est; a.fth_out = fth_out; a.power = power;
  const bool estimate = par->mode == IQ_CR_ESTIMATE;
  const size_t lds = estimate ? ((size_t)2 * a.N + (size_t)2 * a.n2 * a.s1 + 5 * FR_WAVES + 4) * sizeof(float) : 0;
  IQ_PROF_K((double)n_frames * ((double)len * (estimate ? 24 : 16) + (power ? 4.0 * a.N : 0.0)),
            estimate ? (double)n_frames * 8.0 * a.N * (a.n1 + a.n2) : (double)n_frames * len * 6.0, "frames_carrier_kernel");
  launch_frames(frames_carrier_kernel, n_frames, lds, st, a);
  return iq_launch_status();
}

extern "C" int iq_frames_carrier_bwd(const float* dout, float* dx, int n_frames, int len, const iq_carrier_t* par,
                                     iq_stream_t stream) {
  const int rc = check(dout, dx, len, par, true);
  if (rc != IQ_OK) return rc;
  if (n_frames <= 0) return IQ_OK;
  hipStream_t st = (hipStream_t)stream;
  IQ_PROF(IQ_FAM_MISC, st);
  CrArgs a = pack(len, par);
  a.x = dout; a.out = dx;
  IQ_PROF_K((double)n_frames * len * 16, (double)n_frames * len * 6.0, "frames_carrier_bwd_kernel");
  launch_frames(frames_carrier_bwd_kernel, n_frames, 0, st, a);
  return iq_launch_status();
}
