// Cyclic-spectrum front end (iq_frames_cyclic, include/iqvit.h): the spectral correlation function (SCF) of planar (2, len)
// I/Q frames and its conjugate as square (cyclic frequency x frequency) images, by the first stage of the FFT accumulation
// method: the spectrogram's channelizer X[t,k], a per-column phase reference (rot), then the complex Gram matrices over time
//   S[k,l] = sum_t Y[t,k] conj(Y[t,l]),   Sc[k,l] = sum_t Y[t,k] Y[t,l],
// with the power / log / coherence epilogue fused.  Both stages run on the fp32-input MFMA v_mfma_f32_32x32x2_f32 (bit for
// bit a k-ordered fp32 fmaf chain); the channelized frame Y lives in LDS only, nothing but the image goes to HBM.
//
// Decomposition: a band is 32 channels k against all Np channels l.  A band's accumulators (Np/32 tiles of 32 l x 32 k, for each
// of them Re and Im of S and of Sc) stay in registers from the first column to the last: wave w of the four owns the l tiles w
// and w+4.  Time goes through LDS in chunks of 32 columns:
//   stage 1  D[row = bin][col = t] = sum_m A[bin][m] B[m][t], A = the table (read from L2, 32 consecutive bins per row), B =
//            the frame in LDS at its sliding index (channel_step of frames.h); wave w computes the bin tiles w and w+4 of the chunk,
//            applies rot and writes Y[t][bin] (Re plane, Im plane; row stride Np+1 floats: the store has t on the lane and is
//            conflict-free, the reads below have the bin on the lane).  Columns at and behind `columns` are written as zeros.
//   psd      thread b < Np adds |Y[t][b]|^2 of the chunk to its D[b], t ascending.
//   stage 2  tile[row = l][col = k] += sum_t A[l][t] B[t][k], both operands rows of Y: k ends up on the lane, l in the register.
// Two launch shapes, chosen on the host from the LDS need alone, with the same arithmetic in the same order (the images agree bit
// for bit): when every chunk of Y fits in LDS beside the frame (CY_LDS_CACHE bytes: 1024-sample frames with the default hop
// always do) ONE workgroup per frame runs stage 1 once, keeps all of Y, and then runs stage 2 band after band; otherwise one
// workgroup per (frame, band) holds one chunk at a time and every band recomputes the channelizer (Np/32 times the stage-1 work).
// Epilogue: every (k, l) of a band is one element (a, k) of each channel, a = k - l resp. k + l (mod Np).  The values go
// through LDS ([channel][image row][32 band columns]; its own space when Y is kept, the chunk's otherwise) so that the stores
// to HBM are float4s of one image row; no atomics, one writer per element, two runs agree bit for bit.
#include <math.h>

#include "frames.h"
#include "iqvit.h"
#include "prof.h"

namespace {

constexpr int CY_TILE = FR_TILE;                  // MFMA tile edge: bins, channels, and the time columns of a chunk
constexpr int CY_SLOTS = FR_MAX_FFT / CY_TILE / FR_WAVES;   // tiles a wave owns at most: w and w + 4

struct CyArgs {
  const float* x;
  const float* table;
  const float* rot;
  float* out;
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
        const long t = t0 + col;
        const int jw = window_start(t, n, a.p.hop, a.p.pad, len);
        const int ph = window_phase(t, a.p);
        __syncthreads();                                         // frame and rot staged; stage 2 of the previous chunk has read Y
        // ---- stage 1: Y[t][bin] of the chunk, bin tiles wave and wave + 4
#pragma unroll
        for (int u = 0; u < CY_SLOTS; ++u) {
          const int bt = wave + FR_WAVES * u;
          if (bt >= nk) break;                                   // wave-uniform
          const float* tc = a.table + CY_TILE * bt + col;        // c[m][32 bt + col]
          const float* ts = tc + (size_t)n * n;
          f32x16 re = {}, im = {};
          for (int mi = 0; mi < nk; ++mi)
            channel_block(re, im, tc + (size_t)CY_TILE * mi * n, ts + (size_t)CY_TILE * mi * n, n, fI, fQ, jw + CY_TILE * mi, len,
                          half);
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
        __syncthreads();
        // ---- psd
        if (tid < n) {
          for (int tt = 0; tt < tcols; ++tt) {
            const float yr = yre[tt * ys + tid], yi = yim[tt * ys + tid];
            dsum = fmaf(yi, yi, fmaf(yr, yr, dsum));
          }
        }
      }
      // ---- stage 2: the band's Gram tiles; an odd column count ends on a zero row
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
        if (mode == 2) den = __fadd_rn(__fmul_rn(__fmul_rn(dk, psd[l]), inv2), a.p.floor);
        int ch = 0;
        if (SCF) {
          const float P = power(sre[u][r], sim[u][r], inv2);
          const float v = mode == 0 ? P : mode == 1 ? log10f(P + a.p.floor) : P / den;
          int row = k - l + hn;                                  // a = (k - l) mod n, row = (a + n/2) mod n
          row = row < 0 ? row + n : row >= n ? row - n : row;
          vals[(ch * n + row) * CY_TILE + col] = scale_shift(v, a.p.scale, a.p.shift);
          ++ch;
        }
        if (CONJ) {
          const float P = power(cre[u][r], cim[u][r], inv2);
          const float v = mode == 0 ? P : mode == 1 ? log10f(P + a.p.floor) : P / den;
          int row = k + l + hn;                                  // a = (k + l) mod n
          row = row >= 2 * n ? row - 2 * n : row >= n ? row - n : row;
          vals[(ch * n + row) * CY_TILE + col] = scale_shift(v, a.p.scale, a.p.shift);
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

template <bool SCF, bool CONJ>
void launch(const CyArgs& a, int n_frames, bool cached, size_t lds, hipStream_t st) {
  launch_frames(cached ? cyclic_kernel<SCF, CONJ, true> : cyclic_kernel<SCF, CONJ, false>,
                dim3(n_frames, cached ? 1 : a.p.n_fft / CY_TILE), lds, st, a);
}

}  // namespace

extern "C" int iq_frames_cyclic(const float* x, const float* table, const float* rot, float* out, int n_frames, int len,
                                const iq_cyclic_t* p, iq_stream_t stream) {
  // nothing is launched and no pointer dereferenced (other than p) before the checks have passed
  if (!x || !table || !rot || !out || !p) return IQ_ERR_ARG;
  if (len <= 0 || p->hop < 1 || p->columns < 1 || p->pad < 0) return IQ_ERR_ARG;
  if (p->kind < 0 || p->kind > 2 || p->mode < 0 || p->mode > 2) return IQ_ERR_ARG;
  if (!is_finite(p->inv_norm) || !is_finite(p->floor) || !is_finite(p->scale) || !is_finite(p->shift)) return IQ_ERR_ARG;
  if (p->mode != 0 && !(p->floor > 0.f)) return IQ_ERR_ARG;
  if (((uintptr_t)x & 3) || ((uintptr_t)table & 3) || ((uintptr_t)rot & 3) || ((uintptr_t)out & 15)) return IQ_ERR_ARG;
  if (!fft_size_ok(p->n_fft) || !frame_fits(len)) return IQ_ERR_UNSUPPORTED;
  if (n_frames <= 0) return IQ_OK;
  hipStream_t st = (hipStream_t)stream;
  IQ_PROF(IQ_FAM_MISC, st);
  CyArgs a;
  a.x = x; a.table = table; a.rot = rot; a.out = out; a.len = len; a.p = *p;
  a.vec4 = frame_vec4(x, len);
  const int n = p->n_fft, C = p->kind == 2 ? 2 : 1;
  const size_t chunks = ((size_t)p->columns + CY_TILE - 1) / CY_TILE;
  const bool cached = cy_lds_floats(len, n, chunks) * sizeof(float) <= CY_LDS_CACHE;
  // not cached: at most 64 KB + 3 KB + 64.25 KB of the CU's 160 KB
  const size_t lds = cy_lds_floats(len, n, cached ? chunks : 0) * sizeof(float);
  const double cols = (double)n_frames * p->columns;
  IQ_PROF_K((double)n_frames * len * 8 + (double)n_frames * C * n * n * 4 + 8.0 * n * n,
            8.0 * cols * n * n * (cached ? 1 : n / CY_TILE) + 8.0 * C * cols * n * n, "cyclic_kernel<%s, %s, %s>",
            p->kind != 1 ? "true" : "false", p->kind != 0 ? "true" : "false", cached ? "true" : "false");
  if (p->kind == 0) launch<true, false>(a, n_frames, cached, lds, st);
  else if (p->kind == 1) launch<false, true>(a, n_frames, cached, lds, st);
  else launch<true, true>(a, n_frames, cached, lds, st);
  return iq_launch_status();
}
