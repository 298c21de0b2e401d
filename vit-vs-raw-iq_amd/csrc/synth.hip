// Synthetic labelled I/Q frames made on the device (iq_frames_synth, include/iqvit.h): the transmitter in front of the channel of
// impair.hip.  The recipe of data.make_dataset at 1 sample per symbol -- symbols of the frame's class, one carrier phase, unit
// power, complex AWGN at the frame's SNR -- drawn from Philox instead of the host's PCG64, so frame j of a stream is a pure
// function of (seed, stream, j) and a training step gets frames nobody has seen, with no host data and no H2D copy.
//
// One workgroup per frame.  The symbol words go to LDS as integers (a constellation index, a +-1 bit, a 0/1 bit); GMSK runs an
// LDS prefix sum over them (each thread owns a contiguous chunk, the chunk sums are scanned across the workgroup), everything
// stays integer until the table lookup.  The rotated frame is kept in LDS while its power is reduced across the workgroup;
// every thread then scales two consecutive samples, adds their noise and stores them as one 16-byte store, 1 KB per wave.
// Write only: len*8 bytes out per frame (+ 4*len with `symbols`); the Philox rounds (one call per 4 symbols, one per 2 noisy
// samples) and the Box-Muller transforms are VALU work in front of that traffic.
//
// Random numbers: philox4x32 of common.h.  key = (seed lo, seed hi ^ frame hi), counter = (c, frame lo, IQ_SITE_SYNTH, stream)
// with frame = frame_base + blockIdx.x.
//   c = 0xFFFFFFFF      the frame's parameters: word 0 -> theta = 2 pi u24(w); balanced = 0: word 1 -> class, word 2 -> SNR index
//   c = p < 0x80000000  words 4p..4p+3 of the symbol stream; word n belongs to sample n (kind 0), is bit b_n of the GMSK bit
//                       sequence n = 0..len+1 (kind 1) or bit t_n of the OQPSK bit sequence (kind 2: I[n] = t_{n/2},
//                       Q[n] = t_{len/2 + 1 + (n+1)/2})
//   c = 0x80000000 + p  the noise of samples 2p and 2p+1: Box-Muller of words (0,1) and of words (2,3), as impair.hip
// A word w becomes an integer in [0, M) as (uint64(w) * M) >> 32.  Nothing depends on the grid.
#include <math.h>

#include "common.h"
#include "iqvit.h"
#include "prof.h"

namespace {

constexpr int SYN_THREADS = 256;
constexpr int SYN_WAVES = SYN_THREADS / IQ_WAVE;
constexpr uint32_t SYN_PARAM_CTR = 0xFFFFFFFFu;   // never a symbol or noise group: len * 8 <= 64 KB
constexpr uint32_t SYN_NOISE_CTR = 0x80000000u;
constexpr float SYN_TWO_PI = 6.28318530717958647692f;
constexpr float SYN_RSQRT2 = 0.70710678118654752440f;

struct SynArgs {
  float* raw;
  int64_t* labels;
  float* snr;
  float* drawn;
  int32_t* symbols;
  const float2* points;
  int len, n_classes, n_snrs, balanced;
  uint64_t seed, frame_base;
  uint32_t stream;
  int st4;    // every frame of raw starts 16-byte aligned (len even): float4 stores
  iq_synth_class_t classes[IQ_SYNTH_MAX_CLASSES];
  float snrs_db[IQ_SYNTH_MAX_SNRS];
};
static_assert(sizeof(SynArgs) <= 4096, "kernel arguments");

template <bool NOISE>
__global__ __launch_bounds__(SYN_THREADS) void frames_synth_kernel(SynArgs a) {
  // [nq][4] the frame (I,Q interleaved) | [nw][4] the symbol words as integers | 16 (cos, sin) of pi k / 8 | wave sums
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & (IQ_WAVE - 1), wave = tid >> 6, len = a.len;
  const long fi = blockIdx.x;
  const int nq = (len + 1) >> 1;          // sample pairs
  const int nw = (len + 2 + 3) >> 2;      // Philox calls of the symbol stream: len + 2 words
  float2* fr = reinterpret_cast<float2*>(lds);
  int* w = reinterpret_cast<int*>(lds + 4 * nq);
  float2* tab = reinterpret_cast<float2*>(w + 4 * nw);
  float* red = reinterpret_cast<float*>(tab + 16);
  int* wsum = reinterpret_cast<int*>(red + SYN_WAVES);

  // ---- the frame's parameters: every thread derives the same values from the same four words
  const uint64_t frame = a.frame_base + (uint64_t)fi;
  const uint32_t k0 = (uint32_t)a.seed, k1 = (uint32_t)(a.seed >> 32) ^ (uint32_t)(frame >> 32), flo = (uint32_t)frame;
  const u32x4 par = philox4x32(SYN_PARAM_CTR, flo, IQ_SITE_SYNTH, a.stream, k0, k1);
  const float turn = u24(par[0]);
  int cls, si = 0;
  if (a.balanced) {
    cls = (int)(frame % (uint64_t)a.n_classes);
    if (NOISE) si = (int)((frame / (uint64_t)a.n_classes) % (uint64_t)a.n_snrs);
  } else {
    cls = (int)__umulhi(par[1], (uint32_t)a.n_classes);
    if (NOISE) si = (int)__umulhi(par[2], (uint32_t)a.n_snrs);
  }
  const iq_synth_class_t cd = a.classes[cls];
  const int kind = cd.kind;               // frame-uniform: no branch below diverges
  float c0, s0;
  sincospif(2.f * turn, &s0, &c0);

  // ---- symbol words -> integers in LDS
  for (int p = tid; p < nw; p += SYN_THREADS) {
    const u32x4 z = philox4x32((uint32_t)p, flo, IQ_SITE_SYNTH, a.stream, k0, k1);
    int4 v;
    if (kind == 0) {
      v = make_int4((int)__umulhi(z[0], (uint32_t)cd.count), (int)__umulhi(z[1], (uint32_t)cd.count),
                    (int)__umulhi(z[2], (uint32_t)cd.count), (int)__umulhi(z[3], (uint32_t)cd.count));
    } else {
      v = make_int4((int)(z[0] & 1u), (int)(z[1] & 1u), (int)(z[2] & 1u), (int)(z[3] & 1u));
      if (kind == 1) v = make_int4(2 * v.x - 1, 2 * v.y - 1, 2 * v.z - 1, 2 * v.w - 1);
    }
    reinterpret_cast<int4*>(w)[p] = v;
  }
  if (tid < 16) {
    float sn, cs;
    sincospif(0.125f * (float)tid, &sn, &cs);
    tab[tid] = make_float2(cs, sn);
  }
  __syncthreads();

  // ---- GMSK: w[n] <- (sum_{i<=n} b_i + 2 b_{i+1} + b_{i+2}) mod 16, in place.  Thread t owns samples [start, end).
  if (kind == 1) {
    const int chunk = (len + SYN_THREADS - 1) / SYN_THREADS;
    const int start = min(tid * chunk, len), end = min(start + chunk, len);
    int s = 0;
    for (int n = start; n < end; ++n) s += w[n] + 2 * w[n + 1] + w[n + 2];
    const int e0 = w[end], e1 = w[end + 1];      // the next owner overwrites these two: keep them (end + 1 <= len + 1)
    int inc = s;
#pragma unroll
    for (int o = 1; o < IQ_WAVE; o <<= 1) {
      const int t = __shfl_up(inc, o, IQ_WAVE);
      if (lane >= o) inc += t;
    }
    if (lane == IQ_WAVE - 1) wsum[wave] = inc;
    __syncthreads();                             // also: every read above comes before every write below
    int run = inc - s;
    for (int i = 0; i < wave; ++i) run += wsum[i];
    for (int n = start; n < end; ++n) {
      const int b0 = w[n];
      const int b1 = n + 1 < end ? w[n + 1] : e0;
      const int b2 = n + 2 < end ? w[n + 2] : (n + 2 == end ? e0 : e1);
      run += b0 + 2 * b1 + b2;
      w[n] = run & 15;
    }
    __syncthreads();
  }

  // ---- table lookup, carrier phase, power
  const int q0 = (len >> 1) + 1;
  float pw = 0.f;
  for (int n = tid; n < len; n += SYN_THREADS) {
    int sym;
    float2 v;
    if (kind == 0) {
      sym = w[n];
      v = a.points[cd.offset + sym];
    } else if (kind == 1) {
      sym = w[n];
      v = tab[sym];
    } else {
      const int bi = w[n >> 1], bq = w[q0 + ((n + 1) >> 1)];
      sym = 2 * bi + bq;
      v = make_float2(bi ? SYN_RSQRT2 : -SYN_RSQRT2, bq ? SYN_RSQRT2 : -SYN_RSQRT2);
    }
    const float xr = v.x * c0 - v.y * s0, yr = v.x * s0 + v.y * c0;
    fr[n] = make_float2(xr, yr);
    pw = fmaf(yr, yr, fmaf(xr, xr, pw));
    if (a.symbols) a.symbols[fi * len + n] = sym;
  }
  if ((len & 1) && tid == 0) fr[len] = make_float2(0.f, 0.f);     // the second half of the last pair
  pw = wave_sum(pw);
  if (lane == 0) red[wave] = pw;
  __syncthreads();

  const float P = (((red[0] + red[1]) + red[2]) + red[3]) / (float)len;
  const float rs = 1.f / sqrtf(P + 1e-12f);
  float snr = nanf(""), sig = 0.f;
  if (NOISE) {
    snr = a.snrs_db[si];
    sig = sqrtf(0.5f * powf(10.f, -snr / 10.f));
  }
  if (tid == 0) {
    a.labels[fi] = cls;
    a.snr[fi] = snr;
    if (a.drawn) reinterpret_cast<float4*>(a.drawn)[fi] = make_float4((float)cls, snr, SYN_TWO_PI * turn, P);
  }

  // ---- two consecutive samples per thread: normalise, add the noise, one 16-byte store
  float* dst = a.raw + fi * len * 2;
  for (int p = tid; p < nq; p += SYN_THREADS) {
    float4 v = reinterpret_cast<const float4*>(fr)[p];
    v.x *= rs; v.y *= rs; v.z *= rs; v.w *= rs;
    if (NOISE) {
      const u32x4 z = philox4x32(SYN_NOISE_CTR + (uint32_t)p, flo, IQ_SITE_SYNTH, a.stream, k0, k1);
      float g0, g1, g2, g3;
      box_muller(z[0], z[1], g0, g1);
      box_muller(z[2], z[3], g2, g3);
      v.x = fmaf(sig, g0, v.x); v.y = fmaf(sig, g1, v.y);
      v.z = fmaf(sig, g2, v.z); v.w = fmaf(sig, g3, v.w);
    }
    if (a.st4) {
      reinterpret_cast<float4*>(dst)[p] = v;
    } else {
      reinterpret_cast<float2*>(dst)[2 * p] = make_float2(v.x, v.y);
      if (2 * p + 1 < len) reinterpret_cast<float2*>(dst)[2 * p + 1] = make_float2(v.z, v.w);
    }
  }
}

template <bool NOISE>
void launch(const SynArgs& a, int n_frames, size_t lds, hipStream_t st) {
  if (lds > 48 * 1024) (void)hipFuncSetAttribute((const void*)frames_synth_kernel<NOISE>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  frames_synth_kernel<NOISE><<<n_frames, SYN_THREADS, lds, st>>>(a);
}

}  // namespace

extern "C" int iq_frames_synth(float* raw, int64_t* labels, float* snr, float* drawn, int32_t* symbols, int n_frames, int len,
                               const iq_synth_t* par, iq_stream_t stream) {
  if (!raw || !labels || !snr || !par) return IQ_ERR_ARG;
  if (len <= 0) return IQ_ERR_ARG;
  if (!par->classes || par->n_classes <= 0 || par->n_snrs < 0 || (par->n_snrs > 0 && !par->snrs_db)) return IQ_ERR_ARG;
  if (par->balanced & ~1) return IQ_ERR_ARG;
  if (((uintptr_t)raw & 7) || ((uintptr_t)labels & 7) || ((uintptr_t)snr & 3) || ((uintptr_t)drawn & 15) ||
      ((uintptr_t)symbols & 3) || ((uintptr_t)par->points & 7))
    return IQ_ERR_ARG;
  const int nc = par->n_classes < IQ_SYNTH_MAX_CLASSES ? par->n_classes : IQ_SYNTH_MAX_CLASSES;
  for (int i = 0; i < nc; ++i) {
    const iq_synth_class_t& c = par->classes[i];
    if (c.kind < 0 || c.kind > 2) return IQ_ERR_ARG;
    if (c.kind == 0 && (c.count <= 0 || c.offset < 0 || !par->points)) return IQ_ERR_ARG;
  }
  const int ns = par->n_snrs < IQ_SYNTH_MAX_SNRS ? par->n_snrs : IQ_SYNTH_MAX_SNRS;
  for (int i = 0; i < ns; ++i)
    if (!(fabsf(par->snrs_db[i]) < INFINITY)) return IQ_ERR_ARG;
  if ((size_t)len * 8 > 64 * 1024) return IQ_ERR_UNSUPPORTED;
  if (par->n_classes > IQ_SYNTH_MAX_CLASSES || par->n_snrs > IQ_SYNTH_MAX_SNRS) return IQ_ERR_UNSUPPORTED;
  if (n_frames <= 0) return IQ_OK;
  hipStream_t st = (hipStream_t)stream;
  IQ_PROF(IQ_FAM_MISC, st);
  SynArgs a;
  a.raw = raw; a.labels = labels; a.snr = snr; a.drawn = drawn; a.symbols = symbols;
  a.points = reinterpret_cast<const float2*>(par->points);
  a.len = len; a.n_classes = par->n_classes; a.n_snrs = par->n_snrs; a.balanced = par->balanced;
  a.seed = par->seed; a.frame_base = par->frame_base; a.stream = par->stream;
  a.st4 = (len % 2 == 0 && ((uintptr_t)raw & 15) == 0) ? 1 : 0;
  for (int i = 0; i < IQ_SYNTH_MAX_CLASSES; ++i) a.classes[i] = i < par->n_classes ? par->classes[i] : iq_synth_class_t{1, 0, 0};
  for (int i = 0; i < IQ_SYNTH_MAX_SNRS; ++i) a.snrs_db[i] = i < par->n_snrs ? par->snrs_db[i] : 0.f;
  const bool noise = par->n_snrs > 0;
  const size_t lds = (size_t)((len + 1) / 2) * 16 + (size_t)((len + 2 + 3) / 4) * 16 + 16 * sizeof(float2) +
                     SYN_WAVES * (sizeof(float) + sizeof(int));
  const double bytes = (double)n_frames * ((double)len * 8 + 12 + (drawn ? 16 : 0) + (symbols ? (double)len * 4 : 0));
  IQ_PROF_K(bytes, 0.0, "frames_synth_kernel<%s>", noise ? "true" : "false");
  if (noise) launch<true>(a, n_frames, lds, st);
  else launch<false>(a, n_frames, lds, st);
  return iq_launch_status();
}
