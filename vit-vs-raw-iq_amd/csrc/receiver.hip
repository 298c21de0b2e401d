// Receiver for pulse-shaped frames (iq_frames_receive / _bwd, include/iqvit.h): matched filter, one timing estimate per frame,
// one sample per symbol, and the adjoint with the timing held fixed.  One workgroup per frame, the frame in LDS (workgroup
// size, frame limit, launch and the fixed-order sum of the wave sums: frames.h).
//
// Sample-rate pass (E[r], the hot part: len * (J + 1) complex-by-real MACs): a sliding Toeplitz GEMM on the fp32-input MFMA
// v_mfma_f32_16x16x4_f32, per accumulator an fp32 fmaf chain.  A tile is 16 consecutive outputs; a wave takes 16 tiles (256
// outputs) at a time:
//   D[a][c] = sum_t A[a][t] T[t][c],   A[a][t] = x[n0 + 16 a - h + t],   T[t][c] = G[0][t - c] (0 outside [0, J]),
//   so D[a][c] = y(n0 + 16 a + c);  t = 0 .. KP-1, KP = J + 16 rounded up to a multiple of 4.
// Re and Im are two accumulators that share the T operand.  The A rows are runs of the frame 16 samples apart: the frame lies in
// LDS as two planes (Re, Im) at position p = n + h, word p + (p >> 4), with zeros in [0, h) and [len + h, P): the skew puts the
// 16 rows x 4 k of one operand read into 64 different banks, and zero extension costs no select.  T is read from the first table
// row padded with 15 zeros in front and KP - J - 1 behind: lane (c, k) reads word t - c + 15, consecutive over c.  The epilogue
// writes |y(n)|^2, n < len, into LDS; y(n) itself goes nowhere.  Then wave w adds the residues r = w, w + 4, ...: lane l the
// samples n = r + sps (l + 64 i), i ascending, then the butterfly -- a fixed order.
//
// Timing: thread 0 turns E[0 .. sps) into u (and est); everything after reads it from LDS.
// Symbol pass (1 / sps of the work): thread k % 256 computes v[k] as an fmaf chain over row f^ of the table (staged in LDS) and
// the frame planes, keeps it in LDS, the workgroup sums |v|^2 in a fixed order, and every thread stores its symbols scaled.
// Backward: dv[k] into LDS, then thread n % 256 gathers dx[n] over the at most span + 1 symbols whose pulse covers n.
//
// LDS indices.  Planes: the MFMA pass reads p = 256 g + 16 a + t <= 256 (G - 1) + 240 + KP - 1 < P = 256 G + KP, G = groups of
// 256 outputs; the symbol pass reads p = r^ + k sps + j <= sps - 1 + (n_out - 1) sps + J <= len - 1 + J < P.  T: t - c + 15 in
// [0, KP + 15).  Power / symbol region: n < len, k < n_out, max(len, 2 n_out) floats.  u is reduced into [0, sps n_frac) before
// any use, so r^ < sps and f^ < n_frac whatever the caller's array holds.
#include <math.h>

#include "frames.h"
#include "iqvit.h"
#include "prof.h"

namespace {

constexpr int RX_TILE = 16;                        // outputs of one MFMA row
constexpr int RX_GROUP = RX_TILE * RX_TILE;        // outputs of one accumulator pair
constexpr int RX_MAX_SPS = 16, RX_MAX_SPAN = 32, RX_MAX_FRAC = 64;

struct RxArgs {
  const float* raw;     // forward
  float* sym;           // forward
  float* est;
  float* energy;
  const float* dsym;    // backward
  const float* fsym;    // backward: the forward's sym
  const float* fest;    // backward: the forward's est
  float* dx;            // backward
  const float* table;
  const int32_t* u;
  int len, sps, span, n_frac, mode, normalise;
  int J, h, KP, P, n_out;
  int plane;            // floats of one frame plane
  int sample_pass;      // forward: E[r] is needed
};

__device__ __forceinline__ int skew(int p) { return p + (p >> 4); }

__host__ __device__ __forceinline__ int plane_floats(int P) { return (P + (P >> 4) + 4) & ~3; }

// u reduced into [0, sps * n_frac)
__device__ __forceinline__ int wrap_u(int u, int period) {
  u %= period;
  return u < 0 ? u + period : u;
}

__global__ __launch_bounds__(FR_THREADS) void frames_receive_kernel(RxArgs a) {
  // Re plane | Im plane | T words [KP + 16] | table row f^ [J + 4] | |y|^2 [len], later v [n_out][2] | E [16] | red [4] | u, rho
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & (IQ_WAVE - 1), wave = tid >> 6;
  const int len = a.len, sps = a.sps, J = a.J, h = a.h, KP = a.KP, P = a.P, n_out = a.n_out;
  const long fi = blockIdx.x;
  float* xr = lds;
  float* xi = xr + a.plane;
  float* tw = xi + a.plane;
  float* grow = tw + KP + 16;
  float* pw = grow + ((J + 4) & ~3);
  float* E = pw + ((max(len, 2 * n_out) + 3) & ~3);
  float* red = E + 16;
  int* ubox = reinterpret_cast<int*>(red + FR_WAVES);

  // ---- the frame with its zero extension, and the T words
  const float2* src = reinterpret_cast<const float2*>(a.raw) + fi * len;
  for (int p = tid; p < P; p += FR_THREADS) {
    const int n = p - h;
    float2 v = make_float2(0.f, 0.f);
    if (n >= 0 && n < len) v = src[n];
    xr[skew(p)] = v.x;
    xi[skew(p)] = v.y;
  }
  for (int q = tid; q < KP + 16; q += FR_THREADS) {
    const int j = q - (RX_TILE - 1);
    tw[q] = (j >= 0 && j <= J) ? a.table[j] : 0.f;
  }
  if (tid < 16) E[tid] = 0.f;
  __syncthreads();

  if (a.sample_pass) {
    // ---- |y(n)|^2 into pw: 16 tiles of 16 outputs per wave and step
    const int row = lane & 15, kq = lane >> 4;
    const int groups = (len + RX_GROUP - 1) / RX_GROUP;
    for (int g = wave; g < groups; g += FR_WAVES) {
      f32x4 re = {0.f, 0.f, 0.f, 0.f}, im = {0.f, 0.f, 0.f, 0.f};
      const int p0 = RX_GROUP * g + RX_TILE * row + kq;      // A: row `row`, k `kq`
      const int q0 = kq - row + (RX_TILE - 1);               // T: k `kq`, column `row`
      // the operands of step t + 4 are requested before the MFMAs of step t: one wave per SIMD has nothing else to hide the
      // LDS latency behind.  The last step asks for its own operands again (an index inside the planes, a value not used).
      float ar = xr[skew(p0)], ai = xi[skew(p0)], b = tw[q0];
      for (int t = 0; t < KP; t += 4) {
        const int tn = t + 4 < KP ? t + 4 : t;
        const int w = skew(p0 + tn);
        const float nr = xr[w], ni = xi[w], nb = tw[q0 + tn];
        re = __builtin_amdgcn_mfma_f32_16x16x4f32(ar, b, re, 0, 0, 0);
        im = __builtin_amdgcn_mfma_f32_16x16x4f32(ai, b, im, 0, 0, 0);
        ar = nr; ai = ni; b = nb;
      }
      // accumulator register r of lane (c, q) holds row 4 q + r, column c
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int n = RX_GROUP * g + RX_TILE * (4 * kq + r) + row;
        if (n < len) pw[n] = fmaf(im[r], im[r], re[r] * re[r]);
      }
    }
    __syncthreads();
    // ---- E[r]: wave w the residues w, w + 4, ...
    for (int r = wave; r < sps; r += FR_WAVES) {
      float s = 0.f;
      for (int n = r + sps * lane; n < len; n += sps * IQ_WAVE) s += pw[n];
      s = wave_sum(s);
      if (lane == 0) E[r] = s;
    }
    __syncthreads();
    if (a.energy)
      for (int r = tid; r < sps; r += FR_THREADS) a.energy[fi * sps + r] = E[r];
  }

  // ---- timing: one thread
  const int period = sps * a.n_frac;
  if (tid == 0) {
    float xre = 0.f, xim = 0.f, tot = 0.f;
    int best = 0;
    for (int r = 0; r < sps; ++r) {
      float sn, cs;
      sincospif(-2.f * (float)r / (float)sps, &sn, &cs);
      xre = fmaf(E[r], cs, xre);
      xim = fmaf(E[r], sn, xim);
      tot += E[r];
      if (E[r] > E[best]) best = r;
    }
    float t0 = nanf("");
    int u = 0;
    if (a.mode == IQ_RX_GIVEN) {
      u = wrap_u(a.u ? a.u[fi] : 0, period);
    } else if (a.mode == IQ_RX_OERDER_MEYR) {
      t0 = -atan2f(xim, xre) * (float)sps / FR_TWO_PI;
      if (t0 < 0.f) t0 += (float)sps;
      if (t0 >= (float)sps) t0 -= (float)sps;
      if (fabsf(t0) < INFINITY) u = wrap_u((int)rintf(t0 * (float)a.n_frac), period);
    } else {
      t0 = (float)best;
      u = best * a.n_frac;
    }
    ubox[0] = u;
    if (a.est) {
      a.est[4 * fi + 0] = t0;
      a.est[4 * fi + 1] = (float)u;
      a.est[4 * fi + 2] = tot == 0.f ? 0.f : sqrtf(fmaf(xim, xim, xre * xre)) / tot;
    }
  }
  __syncthreads();
  const int u = ubox[0];
  const int rh = u / a.n_frac, fh = u - rh * a.n_frac;
  for (int j = tid; j <= J; j += FR_THREADS) grow[j] = a.table[(size_t)fh * (J + 1) + j];
  __syncthreads();

  // ---- symbols: v[k] = sum_j x[rh + k sps + j - h] G[fh][j]; position p = rh + k sps + j
  float2* vs = reinterpret_cast<float2*>(pw);
  float pv = 0.f;
  for (int k = tid; k < n_out; k += FR_THREADS) {
    const int p0 = rh + k * sps;
    float vr = 0.f, vi = 0.f;
    for (int j = 0; j <= J; ++j) {
      const int w = skew(p0 + j);
      const float g = grow[j];
      vr = fmaf(xr[w], g, vr);
      vi = fmaf(xi[w], g, vi);
    }
    vs[k] = make_float2(vr, vi);
    pv = fmaf(vi, vi, fmaf(vr, vr, pv));
  }
  pv = wave_sum(pv);
  if (lane == 0) red[wave] = pv;
  __syncthreads();
  const float mean = red_sum(red) / (float)n_out;
  const float rs = a.normalise ? 1.f / sqrtf(mean + 1e-12f) : 1.f;
  if (tid == 0 && a.est) a.est[4 * fi + 3] = mean;
  float2* dst = reinterpret_cast<float2*>(a.sym) + fi * n_out;
  for (int k = tid; k < n_out; k += FR_THREADS) {       // every thread reads back what it wrote
    const float2 v = vs[k];
    dst[k] = a.normalise ? make_float2(v.x * rs, v.y * rs) : v;
  }
}

__global__ __launch_bounds__(FR_THREADS) void frames_receive_bwd_kernel(RxArgs a) {
  // dv [n_out][2] | table row f^ [J + 4] | red [4]
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & (IQ_WAVE - 1), wave = tid >> 6;
  const int len = a.len, sps = a.sps, J = a.J, h = a.h, n_out = a.n_out;
  const long fi = blockIdx.x;
  float2* dv = reinterpret_cast<float2*>(lds);
  float* grow = lds + ((2 * n_out + 3) & ~3);
  float* red = grow + ((J + 4) & ~3);
  const int u = wrap_u(a.u ? a.u[fi] : 0, sps * a.n_frac);
  const int rh = u / a.n_frac, fh = u - rh * a.n_frac;
  for (int j = tid; j <= J; j += FR_THREADS) grow[j] = a.table[(size_t)fh * (J + 1) + j];
  const float2* ds = reinterpret_cast<const float2*>(a.dsym) + fi * n_out;
  if (a.normalise) {
    const float2* s = reinterpret_cast<const float2*>(a.fsym) + fi * n_out;
    float dot = 0.f;
    for (int k = tid; k < n_out; k += FR_THREADS) dot = fmaf(ds[k].y, s[k].y, fmaf(ds[k].x, s[k].x, dot));
    dot = wave_sum(dot);
    if (lane == 0) red[wave] = dot;
    __syncthreads();
    const float c = red_sum(red) / (float)n_out;
    const float ir = 1.f / sqrtf(a.fest[4 * fi + 3] + 1e-12f);
    for (int k = tid; k < n_out; k += FR_THREADS)
      dv[k] = make_float2((ds[k].x - s[k].x * c) * ir, (ds[k].y - s[k].y * c) * ir);
  } else {
    for (int k = tid; k < n_out; k += FR_THREADS) dv[k] = ds[k];
  }
  __syncthreads();
  // dx[n] = sum_k dv[k] G[fh][n - k sps - rh + h]: j = i - k sps in [0, J], i = n - rh + h
  float2* dst = reinterpret_cast<float2*>(a.dx) + fi * len;
  for (int n = tid; n < len; n += FR_THREADS) {
    const int i = n - rh + h;                              // >= -(sps - 1)
    int klo = i - J <= 0 ? 0 : (i - J + sps - 1) / sps;
    int khi = i < 0 ? -1 : i / sps;
    if (khi > n_out - 1) khi = n_out - 1;
    float gr = 0.f, gi = 0.f;
    for (int k = klo; k <= khi; ++k) {
      const float g = grow[i - k * sps];
      gr = fmaf(dv[k].x, g, gr);
      gi = fmaf(dv[k].y, g, gi);
    }
    dst[n] = make_float2(gr, gi);
  }
}

// -> IQ_OK or the refusal; nothing is launched and no pointer but par dereferenced before this returns IQ_OK
int check(const void* in, const void* out, int len, const iq_receiver_t* p) {
  if (!in || !out || !p || !p->table) return IQ_ERR_ARG;
  if (len < 1 || p->sps < 1 || p->span < 1 || p->n_frac < 1) return IQ_ERR_ARG;
  if (p->mode < IQ_RX_GIVEN || p->mode > IQ_RX_ENERGY || (p->normalise & ~1)) return IQ_ERR_ARG;
  if (((uintptr_t)in & 7) || ((uintptr_t)out & 7) || ((uintptr_t)p->table & 3) || ((uintptr_t)p->u & 3)) return IQ_ERR_ARG;
  if (p->sps > RX_MAX_SPS || p->span > RX_MAX_SPAN || p->n_frac > RX_MAX_FRAC) return IQ_ERR_UNSUPPORTED;
  if (!frame_fits(len) || len < p->sps) return IQ_ERR_UNSUPPORTED;
  return IQ_OK;
}

RxArgs pack(int len, const iq_receiver_t* p) {
  RxArgs a = {};
  a.table = p->table; a.u = p->u;
  a.len = len; a.sps = p->sps; a.span = p->span; a.n_frac = p->n_frac; a.mode = p->mode; a.normalise = p->normalise;
  a.J = p->sps * p->span;
  a.h = a.J / 2;
  a.KP = (a.J + RX_TILE + 3) & ~3;
  a.P = (len + RX_GROUP - 1) / RX_GROUP * RX_GROUP + a.KP;
  a.n_out = len / p->sps;
  a.plane = plane_floats(a.P);
  return a;
}

}  // namespace

extern "C" int iq_frames_receive(const float* raw, float* sym, float* est, float* energy, int n_frames, int len,
                                 const iq_receiver_t* par, iq_stream_t stream) {
  int rc = check(raw, sym, len, par);
  if (rc == IQ_OK && (((uintptr_t)est & 3) || ((uintptr_t)energy & 3))) rc = IQ_ERR_ARG;
  if (rc == IQ_OK && par->mode == IQ_RX_OERDER_MEYR && par->sps < 3) rc = IQ_ERR_UNSUPPORTED;
  if (rc != IQ_OK) return rc;
  if (n_frames <= 0) return IQ_OK;
  hipStream_t st = (hipStream_t)stream;
  IQ_PROF(IQ_FAM_MISC, st);
  RxArgs a = pack(len, par);
  a.raw = raw; a.sym = sym; a.est = est; a.energy = energy;
  a.sample_pass = (par->mode != IQ_RX_GIVEN || est || energy) ? 1 : 0;
  const int region = len > 2 * a.n_out ? len : 2 * a.n_out;
  const size_t lds = ((size_t)2 * a.plane + a.KP + 16 + ((a.J + 4) & ~3) + ((region + 3) & ~3) + 16 + FR_WAVES + 4) * sizeof(float);
  const double groups = (double)((len + RX_GROUP - 1) / RX_GROUP);
  IQ_PROF_K((double)n_frames * ((double)len * 8 + (double)a.n_out * 8),
            (double)n_frames * (a.sample_pass ? groups * a.KP * 2048.0 : 0.0) + (double)n_frames * a.n_out * (a.J + 1) * 4.0,
            "frames_receive_kernel");
  launch_frames(frames_receive_kernel, n_frames, lds, st, a);
  return iq_launch_status();
}

extern "C" int iq_frames_receive_bwd(const float* dsym, const float* sym, const float* est, float* dx, int n_frames, int len,
                                     const iq_receiver_t* par, iq_stream_t stream) {
  int rc = check(dsym, dx, len, par);
  if (rc == IQ_OK && par->normalise && (!sym || !est)) rc = IQ_ERR_ARG;
  if (rc == IQ_OK && (((uintptr_t)sym & 7) || ((uintptr_t)est & 3))) rc = IQ_ERR_ARG;
  if (rc != IQ_OK) return rc;
  if (n_frames <= 0) return IQ_OK;
  hipStream_t st = (hipStream_t)stream;
  IQ_PROF(IQ_FAM_MISC, st);
  RxArgs a = pack(len, par);
  a.dsym = dsym; a.fsym = sym; a.fest = est; a.dx = dx;
  const size_t lds = ((size_t)((2 * a.n_out + 3) & ~3) + ((a.J + 4) & ~3) + FR_WAVES) * sizeof(float);
  IQ_PROF_K((double)n_frames * ((double)len * 8 + (double)a.n_out * 16), (double)n_frames * len * (par->span + 1) * 4.0,
            "frames_receive_bwd_kernel");
  launch_frames(frames_receive_bwd_kernel, n_frames, lds, st, a);
  return iq_launch_status();
}
