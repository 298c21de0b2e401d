// Cyclic-spectrum front end (iq_frames_cyclic / _bwd, include/iqvit.h): the spectral correlation function (SCF) of planar
// (2, len) I/Q frames and its conjugate as square (cyclic frequency x frequency) images, by the first stage of the FFT
// accumulation method: the spectrogram's channelizer X[t,k], a per-column phase reference (rot), then the complex Gram matrices
// over time
//   S[k,l] = sum_t Y[t,k] conj(Y[t,l]),   Sc[k,l] = sum_t Y[t,k] Y[t,l],
// with the power / log / coherence epilogue fused, and its adjoint.  Every product runs on the fp32-input MFMA
// v_mfma_f32_32x32x2_f32 (bit for bit a k-ordered fp32 fmaf chain); the channelized frame Y lives in LDS only, nothing but the
// image (forward) or the frame's gradient (backward) goes to HBM.
//
// Decomposition: a band is 32 channels k against all Np channels l.  A band's accumulators (Np/32 tiles of 32 l x 32 k, for each
// of them Re and Im of S and of Sc) stay in registers from the first column to the last: wave w of the four owns the l tiles w
// and w+4.  Time goes through LDS in chunks of 32 columns.  The three stages are one definition for both kernels:
//   stage 1  (channelize_chunk) D[row = bin][col = t] = sum_m A[bin][m] B[m][t], A = the table (read from L2, 32 consecutive bins
//            per row), B = the frame in LDS at its sliding index (channel_step of frames.h); wave w computes the bin tiles w and
//            w+4 of the chunk, applies rot and writes Y[t][bin] (Re plane, Im plane; row stride Np+1 floats: the store has t on
//            the lane and is conflict-free, the reads below have the bin on the lane).  Columns at and behind `columns` are
//            written as zeros.
//   psd      (psd_chunk) thread b < Np adds |Y[t][b]|^2 of the chunk to its D[b], t ascending.
//   stage 2  (gram_chunk) tile[row = l][col = k] += sum_t A[l][t] B[t][k], both operands rows of Y: k ends up on the lane, l in
//            the register.
// Forward, two launch shapes, chosen on the host from the LDS need alone, with the same arithmetic in the same order (the images
// agree bit for bit): when every chunk of Y fits in LDS beside the frame (CY_LDS_CACHE bytes: 1024-sample frames with the default
// hop always do) ONE workgroup per frame runs stage 1 once, keeps all of Y, and then runs stage 2 band after band; otherwise one
// workgroup per (frame, band) holds one chunk at a time and every band recomputes the channelizer (Np/32 times the stage-1 work).
// Epilogue: every (k, l) of a band is one element (a, k) of each channel, a = k - l resp. k + l (mod Np).  The values go
// through LDS ([channel][image row][32 band columns]; its own space when Y is kept, the chunk's otherwise) so that the stores
// to HBM are float4s of one image row; no atomics, one writer per element, two runs agree bit for bit.
//
// Backward (cyclic_bwd_kernel): one workgroup per frame, the bands in a loop, dx accumulated in LDS and stored once.  Y is kept
// whole when it fits (the layout of cy_bwd_lds_floats within CY_LDS_MAX), otherwise one chunk at a time is recomputed.  Per band:
//   pass 1   stages 1 and 2 as the forward: the band's S and Sc in registers, D in LDS.  The accumulators then turn into H and Hc
//            in place (the header's u, uc: dout read once along the image row of (k, l) and once along that of (l, k)); the
//            coherence's gD[k] is summed over a lane's registers, then its two lane halves and the four waves in a fixed order.
//   pass 2   per chunk: G_Y[t][k] = sum_l Y[t,l] H[k,l] + conj(Y[t,l]) Hc[k,l].  The accumulator layout of stage 2 IS the B
//            operand layout (register r of lane half h holds row acc_row(r, h), the lane holds k), so H never leaves the
//            registers; A is Y[t = lane][l] from LDS.  Each wave sums over its own l tiles, the four partial tiles are added
//            through LDS as (w0 + w2) + (w1 + w3); then + 2 gD[k] Y[t,k], times rot, and G_X[k][t] stays in LDS.
//   last     G[m][t] = sum_k (c[m,k] + i s[m,k]) G_X[t,k] over the band's 32 channels, four 32-sample window segments at a time
//            (one per wave, the table read from L2), first the I products, then the Q products through LDS into overlap_add of
//            frames.h, the spectrogram backward's gather: thread j % 256 owns sample j of the LDS accumulator.
#include <math.h>

#include "frames.h"
#include "iqvit.h"
#include "prof.h"

namespace {

constexpr int CY_TILE = FR_TILE;                  // MFMA tile edge: bins, channels, and the time columns of a chunk
constexpr int CY_SLOTS = FR_MAX_FFT / CY_TILE / FR_WAVES;   // tiles a wave owns at most: w and w + 4
constexpr int CY_TS = CY_TILE + 1;                // LDS row stride of the backward's 32 x 32 tiles
constexpr int CY_PLANE = CY_TILE * CY_TS;         // floats of one such tile
constexpr float CY_LN10 = 2.30258509299404568402f;

struct CyArgs {
  const float* x;
  const float* table;
  const float* rot;
  float* out;          // forward
  const float* dout;   // backward
  float* dx;           // backward
  int len;
  iq_cyclic_t p;
  int vec4;            // every frame of x starts 16-byte aligned and has a multiple of 4 floats: float4 staging loads
};

__host__ __device__ inline int cy_ystride(int n_fft) { return n_fft + 1; }
__host__ __device__ inline int cy_chunk_floats(int n_fft) { return 2 * CY_TILE * cy_ystride(n_fft); }   // Y [2][32][Np+1]
// floats of LDS: frame [2][len] | rot [2][Np] | psd [Np] | `chunks` chunks of Y | values [2][Np][32]; with chunks = 0 one chunk
// whose space the values take over
__host__ __device__ inline size_t cy_lds_floats(int len, int n_fft, size_t chunks) {
  const size_t fixed = (size_t)frame_floats(len) + 3 * (size_t)n_fft;
  return chunks ? fixed + chunks * cy_chunk_floats(n_fft) + 2 * (size_t)CY_TILE * n_fft : fixed + cy_chunk_floats(n_fft);
}
constexpr size_t CY_LDS_CACHE = 144 * 1024;       // bytes up to which Y is kept whole (the CU has 160 KB)
// the backward: frame [2][len] | dx [2][len] | rot [2][Np] | psd [Np] | gD [32] | gD partials [256] | `chunks` chunks of Y |
// G_X [2][32][33] | four tiles [4][32][33] (the partial G_Y tiles, then the per-column products)
constexpr int CY_BWD_SMALL = CY_TILE + FR_THREADS;
constexpr int CY_BWD_WORK = (2 + FR_WAVES) * CY_PLANE;
__host__ __device__ inline size_t cy_bwd_lds_floats(int len, int n_fft, size_t chunks) {
  return 2 * (size_t)frame_floats(len) + 3 * (size_t)n_fft + CY_BWD_SMALL + chunks * cy_chunk_floats(n_fft) + CY_BWD_WORK;
}
constexpr size_t CY_LDS_MAX = 160 * 1024;         // what one workgroup may have

// j0 mod n_fft of column t, non-negative (j0 = t*hop - pad may be negative)
__device__ __forceinline__ int window_phase(long t, const iq_cyclic_t& p) {
  long r = (t * (long)p.hop - (long)p.pad) % (long)p.n_fft;
  return (int)(r < 0 ? r + p.n_fft : r);
}

// 32 window samples (32*mi ..) of one 32-bin x 32-column tile, the table read from L2: 16 steps of two samples (channel_step)
__device__ __forceinline__ void channel_block(f32x16& re, f32x16& im, const float* tc, const float* ts, int n, const float* fI,
                                              const float* fQ, int j0, int len, int half) {
  float ac[CY_TILE / 2], as[CY_TILE / 2];
#pragma unroll
  for (int s = 0; s < CY_TILE / 2; ++s) {
    ac[s] = tc[(size_t)(2 * s + half) * n];
    as[s] = ts[(size_t)(2 * s + half) * n];
  }
#pragma unroll
  for (int s = 0; s < CY_TILE / 2; ++s) channel_step(re, im, ac[s], as[s], fI, fQ, j0 + 2 * s + half, len);
}

// ---- stage 1: Y[t][bin] of the chunk of columns t0 .. t0 + 31 (tcols of them live), bin tiles wave and wave + 4.  The caller
// holds the barriers: the frame and rot staged and the chunk's space free before, Y complete behind.
__device__ __forceinline__ void channelize_chunk(float* yre, float* yim, const float* table, const float* rc, const float* rs,
                                                 const float* fI, const float* fQ, int len, const iq_cyclic_t& p, long t0,
                                                 int tcols, int wave, int col, int half) {
  const int n = p.n_fft, nk = n / CY_TILE, ys = cy_ystride(n);
  const long t = t0 + col;
  const int jw = window_start(t, n, p.hop, p.pad, len);
  const int ph = window_phase(t, p);
#pragma unroll
  for (int u = 0; u < CY_SLOTS; ++u) {
    const int bt = wave + FR_WAVES * u;
    if (bt >= nk) break;                                   // wave-uniform
    const float* tc = table + CY_TILE * bt + col;          // c[m][32 bt + col]
    const float* ts = tc + (size_t)n * n;
    f32x16 re = {}, im = {};
    for (int mi = 0; mi < nk; ++mi)
      channel_block(re, im, tc + (size_t)CY_TILE * mi * n, ts + (size_t)CY_TILE * mi * n, n, fI, fQ, jw + CY_TILE * mi, len, half);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int bin = CY_TILE * bt + acc_row(r, half);
      const int q = (bin * ph) % n;                        // bin, ph < 256
      const float c = rc[q], s = rs[q];
      const bool live = col < tcols;
      yre[col * ys + bin] = live ? fmaf(im[r], s, re[r] * c) : 0.f;
      yim[col * ys + bin] = live ? fmaf(-re[r], s, im[r] * c) : 0.f;
    }
  }
}

// ---- psd: thread tid < n adds |Y[t][tid]|^2 of the chunk to its dsum, t ascending
__device__ __forceinline__ void psd_chunk(float& dsum, const float* yre, const float* yim, int n, int tcols, int tid) {
  if (tid < n) {
    const int ys = cy_ystride(n);
    for (int tt = 0; tt < tcols; ++tt) {
      const float yr = yre[tt * ys + tid], yi = yim[tt * ys + tid];
      dsum = fmaf(yi, yi, fmaf(yr, yr, dsum));
    }
  }
}

// ---- stage 2: the Gram tiles of the band k0 .. k0 + 31 take one chunk; an odd column count ends on a zero row
template <bool SCF, bool CONJ>
__device__ __forceinline__ void gram_chunk(f32x16 (&sre)[CY_SLOTS], f32x16 (&sim)[CY_SLOTS], f32x16 (&cre)[CY_SLOTS],
                                           f32x16 (&cim)[CY_SLOTS], const float* yre, const float* yim, int n, int k0, int tcols,
                                           int wave, int col, int half) {
  const int nk = n / CY_TILE, ys = cy_ystride(n);
  const int steps = (tcols + 1) >> 1;
#pragma unroll
  for (int u = 0; u < CY_SLOTS; ++u) {
    const int lt = wave + FR_WAVES * u;
    if (lt >= nk) break;                                     // wave-uniform
    for (int s = 0; s < steps; ++s) {
      const int row = (2 * s + half) * ys;
      const float lr = yre[row + CY_TILE * lt + col], li = yim[row + CY_TILE * lt + col];
      const float kr = yre[row + k0 + col], ki = yim[row + k0 + col];
      if (SCF) {                                             // Yk conj(Yl)
        sre[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(lr, kr, sre[u], 0, 0, 0);
        sre[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(li, ki, sre[u], 0, 0, 0);
        sim[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(lr, ki, sim[u], 0, 0, 0);
        sim[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(-li, kr, sim[u], 0, 0, 0);
      }
      if (CONJ) {                                            // Yk Yl
        cre[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(lr, kr, cre[u], 0, 0, 0);
        cre[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(-li, ki, cre[u], 0, 0, 0);
        cim[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(lr, ki, cim[u], 0, 0, 0);
        cim[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(li, kr, cim[u], 0, 0, 0);
      }
    }
  }
}

// the coherence's denominator of (k, l)
__device__ __forceinline__ float coherence_den(float dk, float dl, float inv2, float floor) {
  return __fadd_rn(__fmul_rn(__fmul_rn(dk, dl), inv2), floor);
}

// image row (a + n/2) mod n of cyclic bin a = (k - l) mod n resp. (k + l) mod n
__device__ __forceinline__ int scf_row(int k, int l, int n) {
  const int row = k - l + (n >> 1);
  return row < 0 ? row + n : row >= n ? row - n : row;
}
__device__ __forceinline__ int conj_row(int k, int l, int n) {
  const int row = k + l + (n >> 1);
  return row >= 2 * n ? row - 2 * n : row >= n ? row - n : row;
}

// CACHED: one workgroup per frame keeps every chunk of Y in LDS and loops over the bands; otherwise one per (frame, band)
template <bool SCF, bool CONJ, bool CACHED>
__global__ __launch_bounds__(FR_THREADS) void cyclic_kernel(CyArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & (IQ_WAVE - 1), wave = tid >> 6;
  const int col = lane & 31, half = lane >> 5;
  const int len = a.len, n = a.p.n_fft, T = a.p.columns, nk = n / CY_TILE, ys = cy_ystride(n);
  const long fi = blockIdx.x;
  const int nbands = CACHED ? nk : 1, band0 = CACHED ? 0 : (int)blockIdx.y;
  const int nchunks = (int)(((long)T + CY_TILE - 1) / CY_TILE), chunk_floats = cy_chunk_floats(n);
  const float* fI = lds;
  const float* fQ = lds + len;
  float* rc = lds + frame_floats(len);
  float* rs = rc + n;
  float* psd = rs + n;
  float* ybase = psd + n;
  float* vals = CACHED ? ybase + (size_t)nchunks * chunk_floats : ybase;   // 2 * n * 32 floats <= one chunk's 2 * 32 * (n + 1)
  stage_frame(lds, a.x + fi * 2 * len, len, a.vec4, tid);
  for (int q = tid; q < 2 * n; q += FR_THREADS) rc[q] = a.rot[q];
  constexpr int C = (SCF ? 1 : 0) + (CONJ ? 1 : 0);
  float* img = a.out + (size_t)fi * C * n * n;
  const float inv2 = a.p.inv_norm * a.p.inv_norm;
  const int mode = a.p.mode, hn = n >> 1;
  float dsum = 0.f;                                              // D[tid], tid < n

  for (int bi = 0; bi < nbands; ++bi) {
    const int k0 = CY_TILE * (band0 + bi);                       // the band: channels k0 .. k0 + 31
    const bool produce = bi == 0;                                // this pass makes Y; the later bands of a cached launch read it
    f32x16 sre[CY_SLOTS] = {}, sim[CY_SLOTS] = {}, cre[CY_SLOTS] = {}, cim[CY_SLOTS] = {};
    for (int ci = 0; ci < nchunks; ++ci) {
      const long t0 = (long)ci * CY_TILE;
      const int tcols = (int)(T - t0 < CY_TILE ? T - t0 : CY_TILE);
      float* yre = ybase + (CACHED ? (size_t)ci * chunk_floats : 0);
      float* yim = yre + CY_TILE * ys;
      if (produce) {
        __syncthreads();                                         // frame and rot staged; stage 2 of the previous chunk has read Y
        channelize_chunk(yre, yim, a.table, rc, rs, fI, fQ, len, a.p, t0, tcols, wave, col, half);
        __syncthreads();
        psd_chunk(dsum, yre, yim, n, tcols, tid);
      }
      gram_chunk<SCF, CONJ>(sre, sim, cre, cim, yre, yim, n, k0, tcols, wave, col, half);
    }

    // ---- epilogue: values into LDS as [channel][image row][band column], then rows of float4 to the image
    if (produce && tid < n) psd[tid] = dsum;
    __syncthreads();                      // psd complete; Y of the last chunk read (uncached); the previous band's values stored
    const int k = k0 + col;
    const float dk = psd[k];
#pragma unroll
    for (int u = 0; u < CY_SLOTS; ++u) {
      const int lt = wave + FR_WAVES * u;
      if (lt >= nk) break;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int l = CY_TILE * lt + acc_row(r, half);
        float den = 1.f;
        if (mode == 2) den = coherence_den(dk, psd[l], inv2, a.p.floor);
        int ch = 0;
        if (SCF) {
          const float P = power(sre[u][r], sim[u][r], inv2);
          const float v = mode == 0 ? P : mode == 1 ? log10f(P + a.p.floor) : P / den;
          vals[(ch * n + scf_row(k, l, n)) * CY_TILE + col] = scale_shift(v, a.p.scale, a.p.shift);
          ++ch;
        }
        if (CONJ) {
          const float P = power(cre[u][r], cim[u][r], inv2);
          const float v = mode == 0 ? P : mode == 1 ? log10f(P + a.p.floor) : P / den;
          vals[(ch * n + conj_row(k, l, n)) * CY_TILE + col] = scale_shift(v, a.p.scale, a.p.shift);
        }
      }
    }
    __syncthreads();
    // image column of channel k0 + 4 g is (k0 + 4 g + n/2) mod n; n/2 and k0 are multiples of 16: four columns never straddle the wrap
    for (int q = tid; q < C * n * (CY_TILE / 4); q += FR_THREADS) {
      const int g = q & 7, rw = q >> 3;                          // rw = channel * n + image row
      int kc = k0 + 4 * g + hn;
      kc = kc >= n ? kc - n : kc;
      *reinterpret_cast<float4*>(img + (size_t)rw * n + kc) = *reinterpret_cast<const float4*>(vals + rw * CY_TILE + 4 * g);
    }
  }
}

// One channel's accumulators of a band into H (the header's 2 inv2 u S) in place; -> this lane's part of
// sum_l scale (g[k,l] + g[l,k]) P D[l] / den^2 (coherence, otherwise 0).  g: the channel's dout; conj: rows of a = k + l.
__device__ __forceinline__ float adjoint_weights(f32x16& re, f32x16& im, const float* g, bool conj, int n, int k, int lt,
                                                 int half, const float* psd, float dk, float inv2, const iq_cyclic_t& p) {
  const int hn = n >> 1;
  const int kc = k + hn >= n ? k + hn - n : k + hn;              // image column of channel k
  float gd = 0.f;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int l = CY_TILE * lt + acc_row(r, half);
    const int lc = l + hn >= n ? l + hn - n : l + hn;
    // the element of (k, l): row of a = k -+ l, column of k (consecutive lanes, one row); that of (l, k): column of l
    const int row_kl = conj ? conj_row(k, l, n) : scf_row(k, l, n), row_lk = conj ? row_kl : scf_row(l, k, n);
    const float w = p.scale * (g[(unsigned)(row_kl * n + kc)] + g[(unsigned)(row_lk * n + lc)]);   // < 2^16: 32-bit offsets
    const float P = power(re[r], im[r], inv2);
    float u = w;
    if (p.mode == 1) u = w / (CY_LN10 * (P + p.floor));
    if (p.mode == 2) {
      const float dl = psd[l], den = coherence_den(dk, dl, inv2, p.floor);
      u = w / den;
      gd += w * P * dl / (den * den);
    }
    const float h = 2.f * inv2 * u;
    re[r] *= h;
    im[r] *= h;
  }
  return gd;
}

// CACHED: every chunk of Y stays in LDS; otherwise one chunk at a time is recomputed where it is needed
template <bool SCF, bool CONJ, bool CACHED>
__global__ __launch_bounds__(FR_THREADS) void cyclic_bwd_kernel(CyArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & (IQ_WAVE - 1), wave = tid >> 6;
  const int col = lane & 31, half = lane >> 5;
  const int len = a.len, n = a.p.n_fft, T = a.p.columns, nk = n / CY_TILE, ys = cy_ystride(n);
  const long fi = blockIdx.x;
  const int nchunks = (int)(((long)T + CY_TILE - 1) / CY_TILE), chunk_floats = cy_chunk_floats(n);
  const float* fI = lds;
  const float* fQ = lds + len;
  float* dxa = lds + frame_floats(len);                          // the gradient [2][len]
  float* rc = dxa + frame_floats(len);
  float* rs = rc + n;
  float* psd = rs + n;
  float* gdl = psd + n;                                          // gD of the band's 32 channels
  float* red = gdl + CY_TILE;                                    // its partial sums, one per thread
  float* ybase = red + FR_THREADS;
  float* gx = ybase + (size_t)(CACHED ? nchunks : 1) * chunk_floats;   // G_X [Re, Im][k][t]
  float* tiles = gx + 2 * CY_PLANE;                              // [4][32][33]
  stage_frame(lds, a.x + fi * 2 * len, len, a.vec4, tid);
  for (int q = tid; q < 2 * n; q += FR_THREADS) rc[q] = a.rot[q];
  for (int q = tid; q < 2 * len; q += FR_THREADS) dxa[q] = 0.f;
  constexpr int C = (SCF ? 1 : 0) + (CONJ ? 1 : 0);
  const float* dout = a.dout + (size_t)fi * C * n * n;
  const float inv2 = a.p.inv_norm * a.p.inv_norm;
  const int mode = a.p.mode;
  const long hop = a.p.hop, pad = a.p.pad;
  float dsum = 0.f;                                              // D[tid], tid < n
  int have = -1;                                                 // not CACHED: the chunk that is in LDS

  for (int bi = 0; bi < nk; ++bi) {
    const int k0 = CY_TILE * bi;
    f32x16 sre[CY_SLOTS] = {}, sim[CY_SLOTS] = {}, cre[CY_SLOTS] = {}, cim[CY_SLOTS] = {};
    // ---- pass 1: the band's S and Sc, as the forward
    for (int ci = 0; ci < nchunks; ++ci) {
      const long t0 = (long)ci * CY_TILE;
      const int tcols = (int)(T - t0 < CY_TILE ? T - t0 : CY_TILE);
      float* yre = ybase + (CACHED ? (size_t)ci * chunk_floats : 0);
      float* yim = yre + CY_TILE * ys;
      if (CACHED ? bi == 0 : have != ci) {                       // workgroup-uniform
        __syncthreads();                                         // frame and rot staged; whatever read the chunk's space is done
        channelize_chunk(yre, yim, a.table, rc, rs, fI, fQ, len, a.p, t0, tcols, wave, col, half);
        __syncthreads();
        if (bi == 0) psd_chunk(dsum, yre, yim, n, tcols, tid);
        have = ci;
      }
      gram_chunk<SCF, CONJ>(sre, sim, cre, cim, yre, yim, n, k0, tcols, wave, col, half);
    }
    if (bi == 0 && tid < n) psd[tid] = dsum;
    __syncthreads();                                             // psd complete
    // ---- S, Sc -> H, Hc in place; gD
    {
      const int k = k0 + col;
      const float dk = psd[k];
      float gd = 0.f;
#pragma unroll
      for (int u = 0; u < CY_SLOTS; ++u) {
        const int lt = wave + FR_WAVES * u;
        if (lt >= nk) break;                                     // wave-uniform
        if (SCF) gd += adjoint_weights(sre[u], sim[u], dout, false, n, k, lt, half, psd, dk, inv2, a.p);
        if (CONJ) gd += adjoint_weights(cre[u], cim[u], dout + (SCF ? (size_t)n * n : 0), true, n, k, lt, half, psd, dk, inv2, a.p);
      }
      red[tid] = gd;
      __syncthreads();
      if (tid < CY_TILE) {                                       // lane halves, then the four waves
        float s = 0.f;
        for (int w = 0; w < FR_WAVES; ++w) s += red[IQ_WAVE * w + tid] + red[IQ_WAVE * w + CY_TILE + tid];
        gdl[tid] = -inv2 * s;
      }
    }
    // ---- pass 2
    for (int ci = 0; ci < nchunks; ++ci) {
      const long t0 = (long)ci * CY_TILE;
      const int tcols = (int)(T - t0 < CY_TILE ? T - t0 : CY_TILE);
      float* yre = ybase + (CACHED ? (size_t)ci * chunk_floats : 0);
      float* yim = yre + CY_TILE * ys;
      if (!CACHED && have != ci) {
        __syncthreads();
        channelize_chunk(yre, yim, a.table, rc, rs, fI, fQ, len, a.p, t0, tcols, wave, col, half);
        __syncthreads();
        have = ci;
      }
      // G_Y[row = t][col = k] of this wave's l tiles: A = Y[t][l] from LDS, B = H[k][l] straight from the accumulators
      f32x16 gyr = {}, gyi = {};
#pragma unroll
      for (int u = 0; u < CY_SLOTS; ++u) {
        const int lt = wave + FR_WAVES * u;
        if (lt >= nk) break;                                     // wave-uniform
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int l = CY_TILE * lt + acc_row(r, half);
          const float yr = yre[col * ys + l], yi = yim[col * ys + l];
          if (SCF) {                                             // H Y
            gyr = __builtin_amdgcn_mfma_f32_32x32x2f32(yr, sre[u][r], gyr, 0, 0, 0);
            gyr = __builtin_amdgcn_mfma_f32_32x32x2f32(-yi, sim[u][r], gyr, 0, 0, 0);
            gyi = __builtin_amdgcn_mfma_f32_32x32x2f32(yi, sre[u][r], gyi, 0, 0, 0);
            gyi = __builtin_amdgcn_mfma_f32_32x32x2f32(yr, sim[u][r], gyi, 0, 0, 0);
          }
          if (CONJ) {                                            // Hc conj(Y)
            gyr = __builtin_amdgcn_mfma_f32_32x32x2f32(yr, cre[u][r], gyr, 0, 0, 0);
            gyr = __builtin_amdgcn_mfma_f32_32x32x2f32(yi, cim[u][r], gyr, 0, 0, 0);
            gyi = __builtin_amdgcn_mfma_f32_32x32x2f32(-yi, cre[u][r], gyi, 0, 0, 0);
            gyi = __builtin_amdgcn_mfma_f32_32x32x2f32(yr, cim[u][r], gyi, 0, 0, 0);
          }
        }
      }
      // the four partial tiles as (w0 + w2) + (w1 + w3), [plane][k][t]: waves 0 and 1 store, 2 and 3 add (same lane, same element)
      float* part = tiles + (wave & 1) * 2 * CY_PLANE;
      if (wave < 2) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          part[col * CY_TS + acc_row(r, half)] = gyr[r];
          part[CY_PLANE + col * CY_TS + acc_row(r, half)] = gyi[r];
        }
      }
      __syncthreads();                                           // (also: gdl is written)
      if (wave >= 2) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          part[col * CY_TS + acc_row(r, half)] += gyr[r];
          part[CY_PLANE + col * CY_TS + acc_row(r, half)] += gyi[r];
        }
      }
      __syncthreads();
      // + 2 gD[k] Y[t,k], times rot: G_X = (rc + i rs) G_Y, the transpose of the forward's rotation
      for (int e = tid; e < CY_TILE * CY_TILE; e += FR_THREADS) {
        const int t = e & 31, kk = e >> 5, o = kk * CY_TS + t;
        float gr = tiles[o] + tiles[2 * CY_PLANE + o], gi = tiles[CY_PLANE + o] + tiles[3 * CY_PLANE + o];
        if (mode == 2) {
          const float g2 = 2.f * gdl[kk];
          gr = fmaf(g2, yre[t * ys + k0 + kk], gr);
          gi = fmaf(g2, yim[t * ys + k0 + kk], gi);
        }
        const int q = ((k0 + kk) * window_phase(t0 + t, a.p)) % n;
        const float c = rc[q], s = rs[q];
        gx[o] = gr * c - gi * s;
        gx[CY_PLANE + o] = gr * s + gi * c;
      }
      __syncthreads();                                           // G_X complete, the four tiles free
      // ---- G_I[m][t] = sum_k c dRe - s dIm,  G_Q[m][t] = sum_k s dRe + c dIm over the band: one 32-sample segment per wave
      for (int ms = 0; ms * FR_WAVES < nk; ++ms) {
        const int mi = ms * FR_WAVES + wave;
        const bool has_m = mi < nk;                              // wave-uniform
        f32x16 pi = {}, pq = {};
        if (has_m) {
          const float* tc = a.table + (size_t)(CY_TILE * mi + col) * n + k0 + half;   // c[32 mi + col][k0 + 2 s + half]
          const float* ts = tc + (size_t)n * n;
#pragma unroll 4
          for (int s = 0; s < CY_TILE / 2; ++s) {
            const float ac = tc[2 * s], as = ts[2 * s];
            const float br = gx[(2 * s + half) * CY_TS + col], bq = gx[CY_PLANE + (2 * s + half) * CY_TS + col];
            pi = __builtin_amdgcn_mfma_f32_32x32x2f32(ac, br, pi, 0, 0, 0);
            pi = __builtin_amdgcn_mfma_f32_32x32x2f32(-as, bq, pi, 0, 0, 0);
            pq = __builtin_amdgcn_mfma_f32_32x32x2f32(as, br, pq, 0, 0, 0);
            pq = __builtin_amdgcn_mfma_f32_32x32x2f32(ac, bq, pq, 0, 0, 0);
          }
        }
        const long mlo = (long)ms * FR_WAVES * CY_TILE;
        const long mhi = mlo + FR_WAVES * CY_TILE < n ? mlo + FR_WAVES * CY_TILE : (long)n;
        float* mine = tiles + wave * CY_PLANE;
        if (has_m) {
#pragma unroll
          for (int r = 0; r < 16; ++r) mine[acc_row(r, half) * CY_TS + col] = pi[r];
        }
        __syncthreads();
        overlap_add<1>(dxa, nullptr, tiles, CY_PLANE, CY_TS, 0, t0, tcols, hop, pad, mlo, mhi, len, tid);
        __syncthreads();
        if (has_m) {
#pragma unroll
          for (int r = 0; r < 16; ++r) mine[acc_row(r, half) * CY_TS + col] = pq[r];
        }
        __syncthreads();
        overlap_add<1>(dxa + len, nullptr, tiles, CY_PLANE, CY_TS, 0, t0, tcols, hop, pad, mlo, mhi, len, tid);
        __syncthreads();                                         // the four tiles free again
      }
    }
  }
  // every element of dx once; the syncs above order the last additions before these reads
  float* dx = a.dx + fi * 2 * len;
  for (int q = tid; q < 2 * len; q += FR_THREADS) dx[q] = dxa[q];
}

template <bool SCF, bool CONJ>
void launch(const CyArgs& a, int n_frames, bool cached, size_t lds, hipStream_t st) {
  launch_frames(cached ? cyclic_kernel<SCF, CONJ, true> : cyclic_kernel<SCF, CONJ, false>,
                dim3(n_frames, cached ? 1 : a.p.n_fft / CY_TILE), lds, st, a);
}

template <bool SCF, bool CONJ>
void launch_bwd(const CyArgs& a, int n_frames, bool cached, size_t lds, hipStream_t st) {
  launch_frames(cached ? cyclic_bwd_kernel<SCF, CONJ, true> : cyclic_bwd_kernel<SCF, CONJ, false>, dim3(n_frames), lds, st, a);
}

// -> IQ_OK or the refusal; nothing is launched and no pointer dereferenced (other than p) before this returns IQ_OK.  io: out
// (16-byte aligned), or dout and dx (4-byte aligned)
int check(const void* x, const void* table, const void* rot, const void* io_a, const void* io_b, unsigned io_mask, int len,
          const iq_cyclic_t* p) {
  if (!x || !table || !rot || !io_a || !io_b || !p) return IQ_ERR_ARG;
  if (len <= 0 || p->hop < 1 || p->columns < 1 || p->pad < 0) return IQ_ERR_ARG;
  if (p->kind < 0 || p->kind > 2 || p->mode < 0 || p->mode > 2) return IQ_ERR_ARG;
  if (!is_finite(p->inv_norm) || !is_finite(p->floor) || !is_finite(p->scale) || !is_finite(p->shift)) return IQ_ERR_ARG;
  if (p->mode != 0 && !(p->floor > 0.f)) return IQ_ERR_ARG;
  if (((uintptr_t)x & 3) || ((uintptr_t)table & 3) || ((uintptr_t)rot & 3) || ((uintptr_t)io_a & io_mask) ||
      ((uintptr_t)io_b & io_mask))
    return IQ_ERR_ARG;
  if (!fft_size_ok(p->n_fft) || !frame_fits(len)) return IQ_ERR_UNSUPPORTED;
  return IQ_OK;
}

CyArgs pack(const float* x, const float* table, const float* rot, int len, const iq_cyclic_t* p) {
  CyArgs a;
  a.x = x; a.table = table; a.rot = rot; a.out = nullptr; a.dout = nullptr; a.dx = nullptr; a.len = len; a.p = *p;
  a.vec4 = frame_vec4(x, len);
  return a;
}

const char* flag(bool b) { return b ? "true" : "false"; }

}  // namespace

extern "C" int iq_frames_cyclic(const float* x, const float* table, const float* rot, float* out, int n_frames, int len,
                                const iq_cyclic_t* p, iq_stream_t stream) {
  const int rc = check(x, table, rot, out, out, 15, len, p);
  if (rc != IQ_OK) return rc;
  if (n_frames <= 0) return IQ_OK;
  hipStream_t st = (hipStream_t)stream;
  IQ_PROF(IQ_FAM_MISC, st);
  CyArgs a = pack(x, table, rot, len, p);
  a.out = out;
  const int n = p->n_fft, C = p->kind == 2 ? 2 : 1;
  const size_t chunks = ((size_t)p->columns + CY_TILE - 1) / CY_TILE;
  const bool cached = cy_lds_floats(len, n, chunks) * sizeof(float) <= CY_LDS_CACHE;
  // not cached: at most 64 KB + 3 KB + 64.25 KB of the CU's 160 KB
  const size_t lds = cy_lds_floats(len, n, cached ? chunks : 0) * sizeof(float);
  const double cols = (double)n_frames * p->columns;
  IQ_PROF_K((double)n_frames * len * 8 + (double)n_frames * C * n * n * 4 + 8.0 * n * n,
            8.0 * cols * n * n * (cached ? 1 : n / CY_TILE) + 8.0 * C * cols * n * n, "cyclic_kernel<%s, %s, %s>",
            flag(p->kind != 1), flag(p->kind != 0), flag(cached));
  if (p->kind == 0) launch<true, false>(a, n_frames, cached, lds, st);
  else if (p->kind == 1) launch<false, true>(a, n_frames, cached, lds, st);
  else launch<true, true>(a, n_frames, cached, lds, st);
  return iq_launch_status();
}

extern "C" int iq_frames_cyclic_bwd(const float* x, const float* table, const float* rot, const float* dout, float* dx,
                                    int n_frames, int len, const iq_cyclic_t* p, iq_stream_t stream) {
  const int rc = check(x, table, rot, dout, dx, 3, len, p);
  if (rc != IQ_OK) return rc;
  // the frame, its gradient and one chunk of Y beside the working tiles: above the CU's LDS for the longest frames
  if (cy_bwd_lds_floats(len, p->n_fft, 1) * sizeof(float) > CY_LDS_MAX) return IQ_ERR_UNSUPPORTED;
  if (n_frames <= 0) return IQ_OK;
  hipStream_t st = (hipStream_t)stream;
  IQ_PROF(IQ_FAM_MISC, st);
  CyArgs a = pack(x, table, rot, len, p);
  a.dout = dout; a.dx = dx;
  const int n = p->n_fft, C = p->kind == 2 ? 2 : 1;
  const size_t chunks = ((size_t)p->columns + CY_TILE - 1) / CY_TILE;
  const bool cached = cy_bwd_lds_floats(len, n, chunks) * sizeof(float) <= CY_LDS_MAX;
  const size_t lds = cy_bwd_lds_floats(len, n, cached ? chunks : 1) * sizeof(float);
  const double cols = (double)n_frames * p->columns;
  // stage 1 once (twice per band when Y is recomputed), stage 2 and its transpose per channel, the table's transpose
  IQ_PROF_K((double)n_frames * len * 16 + 2.0 * n_frames * C * n * n * 4 + 16.0 * n * n,
            8.0 * cols * n * n * (cached ? 1 : 2 * n / CY_TILE) + 16.0 * C * cols * n * n + 8.0 * cols * n * n,
            "cyclic_bwd_kernel<%s, %s, %s>", flag(p->kind != 1), flag(p->kind != 0), flag(cached));
  if (p->kind == 0) launch_bwd<true, false>(a, n_frames, cached, lds, st);
  else if (p->kind == 1) launch_bwd<false, true>(a, n_frames, cached, lds, st);
  else launch_bwd<true, true>(a, n_frames, cached, lds, st);
  return iq_launch_status();
}
