// Synthetic labelled I/Q frames made on the device (iq_frames_synth, include/iqvit.h): the transmitter in front of the channel of
// impair.hip.  The recipe of data.make_dataset at 1 sample per symbol -- symbols of the frame's class, one carrier phase, unit
// power, complex AWGN at the frame's SNR -- drawn from Philox instead of the host's PCG64, so frame j of a stream is a pure
// function of (seed, stream, j) and a training step gets frames nobody has seen, with no host data and no H2D copy.
//
// One workgroup per frame.  The symbol words go to LDS as integers (a constellation index, a +-1 bit, a 0/1 bit); GMSK runs an
// LDS prefix sum over them (each thread owns a contiguous chunk, the chunk sums are scanned across the workgroup), everything
// stays integer until the table lookup.  The rotated frame is kept in LDS; the tail (power, unit scale, noise, 16-byte stores,
// 1 KB per wave) is frames.h's frame_scale + store_frame, as are the keying, the class / SNR draw and the rotation.
// Write only: len*8 bytes out per frame (+ 4*len with `symbols`); the Philox rounds (one call per 4 symbols, one per 2 noisy
// samples) and the Box-Muller transforms are VALU work in front of that traffic.
//
// Random numbers: philox4x32 of common.h.  key = (seed lo, seed hi ^ frame hi), counter = (c, frame lo, IQ_SITE_SYNTH, stream)
// with frame = frame_base + blockIdx.x.
//   c = 0xFFFFFFFF      the frame's parameters: word 0 -> theta = 2 pi u24(w); balanced = 0: word 1 -> class, word 2 -> SNR index
//   c = p < 0x80000000  words 4p..4p+3 of the symbol stream; word n belongs to sample n (kind 0), is bit b_n of the GMSK bit
//                       sequence n = 0..len+1 (kind 1) or bit t_n of the OQPSK bit sequence (kind 2: I[n] = t_{n/2},
//                       Q[n] = t_{len/2 + 1 + (n+1)/2})
//   c = 0x80000000 + p  the noise of samples 2p and 2p+1 (noise4)
// A word w becomes an integer in [0, M) as (uint64(w) * M) >> 32.  Nothing depends on the grid.
#include <math.h>

#include "frames.h"
#include "iqvit.h"
#include "prof.h"

namespace {

constexpr uint32_t SYN_NOISE_CTR = 0x80000000u;

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
__global__ __launch_bounds__(FR_THREADS) void frames_synth_kernel(SynArgs a) {
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
  int* wsum = reinterpret_cast<int*>(red + FR_WAVES);

  // ---- the frame's parameters: every thread derives the same values from the same four words
  const FrameKey key = frame_key(a.seed, a.frame_base, blockIdx.x);
  const uint32_t k0 = key.k0, k1 = key.k1, flo = key.flo;
  const u32x4 par = philox4x32(FR_PARAM_CTR, flo, IQ_SITE_SYNTH, a.stream, k0, k1);
  const float turn = u24(par[0]);
  int cls, si;
  draw_class_snr(key.frame, par, a.balanced, a.n_classes, a.n_snrs, NOISE, cls, si);
  const iq_synth_class_t cd = a.classes[cls];
  const int kind = cd.kind;               // frame-uniform: no branch below diverges
  float c0, s0;
  sincospif(2.f * turn, &s0, &c0);

  // ---- symbol words -> integers in LDS
  for (int p = tid; p < nw; p += FR_THREADS) {
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
    const int chunk = (len + FR_THREADS - 1) / FR_THREADS;
    const int start = min(tid * chunk, len), end = min(start + chunk, len);
    int s = 0;
    for (int n = start; n < end; ++n) s += w[n] + 2 * w[n + 1] + w[n + 2];
    const int e0 = w[end], e1 = w[end + 1];      // the next owner overwrites these two: keep them (end + 1 <= len + 1)
    int run = scan_exclusive(s, wsum, lane, wave);   // its barrier: every read above comes before every write below
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
  for (int n = tid; n < len; n += FR_THREADS) {
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
      v = make_float2(bi ? FR_RSQRT2 : -FR_RSQRT2, bq ? FR_RSQRT2 : -FR_RSQRT2);
    }
    const float2 r = rotate(v, c0, s0);
    fr[n] = r;
    pw = fmaf(r.y, r.y, fmaf(r.x, r.x, pw));
    if (a.symbols) a.symbols[fi * len + n] = sym;
  }
  if ((len & 1) && tid == 0) fr[len] = make_float2(0.f, 0.f);     // the second half of the last pair
  const float snr = NOISE ? a.snrs_db[si] : nanf("");
  const FrameScale f = frame_scale(pw, red, len, lane, wave, NOISE, snr);
  if (tid == 0) {
    a.labels[fi] = cls;
    a.snr[fi] = snr;
    if (a.drawn) reinterpret_cast<float4*>(a.drawn)[fi] = make_float4((float)cls, snr, FR_TWO_PI * turn, f.P);
  }
  store_frame(a.raw + fi * len * 2, fr, len, a.st4, tid, f, NOISE, SYN_NOISE_CTR, flo, IQ_SITE_SYNTH, a.stream, k0, k1);
}

}  // namespace

extern "C" int iq_frames_synth(float* raw, int64_t* labels, float* snr, float* drawn, int32_t* symbols, int n_frames, int len,
                               const iq_synth_t* par, iq_stream_t stream) {
  if (!raw || !labels || !snr || !par) return IQ_ERR_ARG;
  if (len <= 0) return IQ_ERR_ARG;
  if (!synth_lists_ok(par->classes, par->n_classes, par->snrs_db, par->n_snrs, par->points, par->balanced)) return IQ_ERR_ARG;
  if (((uintptr_t)raw & 7) || ((uintptr_t)labels & 7) || ((uintptr_t)snr & 3) || ((uintptr_t)drawn & 15) ||
      ((uintptr_t)symbols & 3) || ((uintptr_t)par->points & 7))
    return IQ_ERR_ARG;
  if (!frame_fits(len)) return IQ_ERR_UNSUPPORTED;
  if (par->n_classes > IQ_SYNTH_MAX_CLASSES || par->n_snrs > IQ_SYNTH_MAX_SNRS) return IQ_ERR_UNSUPPORTED;
  if (n_frames <= 0) return IQ_OK;
  hipStream_t st = (hipStream_t)stream;
  IQ_PROF(IQ_FAM_MISC, st);
  SynArgs a;
  a.raw = raw; a.labels = labels; a.snr = snr; a.drawn = drawn; a.symbols = symbols;
  a.points = reinterpret_cast<const float2*>(par->points);
  a.len = len; a.n_classes = par->n_classes; a.n_snrs = par->n_snrs; a.balanced = par->balanced;
  a.seed = par->seed; a.frame_base = par->frame_base; a.stream = par->stream;
  a.st4 = frame_vec4(raw, len);
  pack_synth_lists(a.classes, a.snrs_db, par->classes, par->n_classes, par->snrs_db, par->n_snrs);
  const bool noise = par->n_snrs > 0;
  const size_t lds = (size_t)((len + 1) / 2) * 16 + (size_t)((len + 2 + 3) / 4) * 16 + 16 * sizeof(float2) +
                     FR_WAVES * (sizeof(float) + sizeof(int));
  const double bytes = (double)n_frames * ((double)len * 8 + 12 + (drawn ? 16 : 0) + (symbols ? (double)len * 4 : 0));
  IQ_PROF_K(bytes, 0.0, "frames_synth_kernel<%s>", noise ? "true" : "false");
  launch_frames(noise ? frames_synth_kernel<true> : frames_synth_kernel<false>, n_frames, lds, st, a);
  return iq_launch_status();
}
