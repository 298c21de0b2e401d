// Spectrogram front end (iq_frames_spectrogram / _bwd, include/iqvit.h): the short-time Fourier transform of planar (2, len)
// I/Q frames as a sliding complex GEMM against a caller-supplied (c, s) table, with the power / log epilogue fused, and its
// adjoint.  The image [n_fft rows = frequency bins in fftshift order][width columns = time] is what the ViT reads.
//
// Arithmetic: the fp32-input MFMA v_mfma_f32_32x32x2_f32 -- bit for bit a k-ordered fp32 fmaf chain, at the fp32 matrix rate.
// (A bf16 MFMA would put a floor near -48 dB under the strongest bin, inside the range a log image shows.)
// Orientation: D[row = bin][col = t] = sum_m A[bin][m] * B[m][t], A = the table, B[m][t] = frame[t*hop - pad + m].  The
// accumulator then has t on the lane (col = lane & 31) and the bin in the register, Re and Im of one (bin, t) sit in the same
// lane and register of two accumulators, the epilogue needs no exchange, and every store is 32 consecutive floats of one row.
// The B operand is read from the frame in LDS at its sliding index (no im2col copy); samples outside [0, len) are a select of
// 0, never a read.  The A operand comes from a 32 x 32 block of c and of s staged in LDS (row stride 33 floats: conflict-free
// for the forward's row read and for the backward's transposed read); at most 2*256*256*4 B = 512 KB, the table stays in L2.
// Nothing of size width * n_fft * 2 goes to HBM.  The frame staging, the window start, the four-MFMA step, the accumulator
// layout and the image value are the channelizer stages of frames.h, shared with cyclic.hip.
//
// Forward: one workgroup per (frame, 32 image rows), four waves; wave w owns time tiles w and w+4 of every 256 columns, so
// all four share the table block.  The next block is loaded into registers under the MFMAs of the current one.
//
// Backward: one workgroup per frame, simpler and slower.  Per tile of 32 columns and per group of four row tiles (one per
// wave): recompute Re / Im, turn them into dRe / dIm ([128][32] in LDS), then per group of four 32-sample window segments (one
// per wave) multiply by the transposed table, leave the per-column products G[m][t] in LDS, and let thread j % 256 add to
// dx[j] the products of the columns that cover sample j, in ascending t.  Every dx element is read and written by one thread
// only, in program order: no atomics, no dependence on timing, two runs agree bit for bit.
#include <math.h>

#include "frames.h"
#include "iqvit.h"
#include "prof.h"

namespace {

constexpr int SP_TILE = FR_TILE;                  // MFMA tile edge: image rows, time columns, window samples per block
constexpr int SP_TS = SP_TILE + 1;                // LDS row stride of a staged block and of the G products
constexpr int SP_BLOCK = 2 * SP_TILE * SP_TS;     // floats of one block: c[32][33] then s[32][33]
constexpr int SP_DROWS = FR_WAVES * SP_TILE;      // rows of dRe / dIm the backward holds at a time
constexpr float SP_LN10 = 2.30258509299404568402f;

struct SpArgs {
  const float* x;
  const float* table;
  float* out;          // forward
  const float* dout;   // backward
  float* dx;           // backward
  int len;
  iq_spectrogram_t p;
  int vec4;            // every frame of x starts 16-byte aligned and has a multiple of 4 floats: float4 staging loads
};

// Element q (of 512) of the block (window samples 32*mi .., image rows 32*ki ..): plane q >> 8, sample (q >> 3) & 31, four
// consecutive rows from 4 * (q & 7).  Image row r holds bin (r + n_fft/2) mod n_fft; n_fft/2 is a multiple of 16, so four
// rows from a multiple of 4 never straddle the wrap.
__device__ __forceinline__ float4 block_load(const float* table, int n_fft, int mi, int ki, int q) {
  const int pl = q >> 8, r = (q >> 3) & 31, c4 = (q & 7) * 4;
  int bin = SP_TILE * ki + c4 + (n_fft >> 1);
  if (bin >= n_fft) bin -= n_fft;
  return *reinterpret_cast<const float4*>(table + ((size_t)pl * n_fft + SP_TILE * mi + r) * n_fft + bin);
}
__device__ __forceinline__ void block_store(float* blk, int q, float4 v) {
  float* d = blk + ((q >> 8) * SP_TILE + ((q >> 3) & 31)) * SP_TS + (q & 7) * 4;
  d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
}

// 32 window samples of one 32-bin x 32-column tile from a staged block: 16 steps of two samples (channel_step)
__device__ __forceinline__ void tile_block(f32x16& re, f32x16& im, const float* blk, const float* fI, const float* fQ, int j0,
                                           int len, int col, int half) {
#pragma unroll
  for (int s = 0; s < SP_TILE / 2; ++s) {
    const int mm = 2 * s + half;
    channel_step(re, im, blk[mm * SP_TS + col], blk[(SP_TILE + mm) * SP_TS + col], fI, fQ, j0 + mm, len);
  }
}

__device__ __forceinline__ void store_tile(const f32x16& re, const f32x16& im, float* out_rows, int W, int t,
                                           const iq_spectrogram_t& p, int half) {
  if (t >= W) return;
#pragma unroll
  for (int r = 0; r < 16; ++r)
    out_rows[(size_t)acc_row(r, half) * W + t] = image_value(re[r], im[r], p.inv_norm, p.mode, p.floor, p.scale, p.shift);
}

__global__ __launch_bounds__(FR_THREADS) void spectrogram_fwd_kernel(SpArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];   // the frame [2][len], then one table block
  const int tid = threadIdx.x, lane = tid & (IQ_WAVE - 1), wave = tid >> 6;
  const int col = lane & 31, half = lane >> 5;
  const int len = a.len, n = a.p.n_fft, W = a.p.width, nk = n / SP_TILE;
  const long fi = blockIdx.x;
  const int ki = blockIdx.y;
  const float* fI = lds;
  const float* fQ = lds + len;
  float* blk = lds + frame_floats(len);
  stage_frame(lds, a.x + fi * 2 * len, len, a.vec4, tid);
  float* out_rows = a.out + ((size_t)fi * n + (size_t)SP_TILE * ki) * W;

  for (long tg = 0; tg < W; tg += 2 * FR_WAVES * SP_TILE) {
    const long ta = tg + SP_TILE * wave, tb = ta + FR_WAVES * SP_TILE;
    const bool has_a = ta < W, has_b = tb < W;                  // wave-uniform
    const int ja = window_start(ta + col, n, a.p.hop, a.p.pad, len), jb = window_start(tb + col, n, a.p.hop, a.p.pad, len);
    f32x16 re_a = {}, im_a = {}, re_b = {}, im_b = {};
    float4 pre0 = block_load(a.table, n, 0, ki, tid), pre1 = block_load(a.table, n, 0, ki, tid + FR_THREADS);
    for (int mi = 0; mi < nk; ++mi) {
      __syncthreads();                                          // the previous block has been read (first pass: nothing)
      block_store(blk, tid, pre0);
      block_store(blk, tid + FR_THREADS, pre1);
      __syncthreads();                                          // block mi (and, first pass, the frame) is in LDS
      if (mi + 1 < nk) {
        pre0 = block_load(a.table, n, mi + 1, ki, tid);
        pre1 = block_load(a.table, n, mi + 1, ki, tid + FR_THREADS);
      }
      if (has_a) tile_block(re_a, im_a, blk, fI, fQ, ja + SP_TILE * mi, len, col, half);
      if (has_b) tile_block(re_b, im_b, blk, fI, fQ, jb + SP_TILE * mi, len, col, half);
    }
    if (has_a) store_tile(re_a, im_a, out_rows, W, (int)ta + col, a.p, half);
    if (has_b) store_tile(re_b, im_b, out_rows, W, (int)tb + col, a.p, half);
  }
}

__global__ __launch_bounds__(FR_THREADS) void spectrogram_bwd_kernel(SpArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];   // frame [2][len] | dRe, dIm [2][128][32] | 4 blocks (then G)
  const int tid = threadIdx.x, lane = tid & (IQ_WAVE - 1), wave = tid >> 6;
  const int col = lane & 31, half = lane >> 5;
  const int len = a.len, n = a.p.n_fft, W = a.p.width, nk = n / SP_TILE;
  const long hop = a.p.hop, pad = a.p.pad;
  const long fi = blockIdx.x;
  const float* fI = lds;
  const float* fQ = lds + len;
  float* dre = lds + frame_floats(len);
  float* dim = dre + SP_DROWS * SP_TILE;
  float* blocks = dim + SP_DROWS * SP_TILE;
  float* blk = blocks + wave * SP_BLOCK;                         // this wave's table block, later its G[2][32][33]
  stage_frame(lds, a.x + fi * 2 * len, len, a.vec4, tid);
  float* dxi = a.dx + fi * 2 * len;
  float* dxq = dxi + len;
  for (int j = tid; j < len; j += FR_THREADS) dxi[j] = dxq[j] = 0.f;   // thread j % 256 owns sample j from here on
  const float* dout = a.dout + (size_t)fi * n * W;

  for (long t0 = 0; t0 < W; t0 += SP_TILE) {
    const long t = t0 + col;
    const int jw = window_start(t, n, a.p.hop, a.p.pad, len);
    const int tcols = (int)(W - t0 < SP_TILE ? W - t0 : SP_TILE);
    for (int ks = 0; ks * FR_WAVES < nk; ++ks) {
      // ---- recompute Re / Im of image rows 32*ki .. of this column tile, one row tile per wave
      const int ki = ks * FR_WAVES + wave;
      const bool has_k = ki < nk;                               // wave-uniform
      f32x16 re = {}, im = {};
      for (int mi = 0; mi < nk; ++mi) {
        __syncthreads();                                        // blocks / G of the previous step have been read
        if (has_k)
          for (int q = lane; q < 512; q += IQ_WAVE) block_store(blk, q, block_load(a.table, n, mi, ki, q));
        __syncthreads();
        if (has_k) tile_block(re, im, blk, fI, fQ, jw + SP_TILE * mi, len, col, half);
      }
      // ---- dRe = 2 Re g, dIm = 2 Im g, g = dout * dout/dP
      if (has_k) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = acc_row(r, half);
          float g = 0.f;
          if (t < W) {
            g = dout[((size_t)SP_TILE * ki + row) * W + t] * a.p.scale * a.p.inv_norm;
            if (a.p.mode) g = g / (SP_LN10 * (power(re[r], im[r], a.p.inv_norm) + a.p.floor));
          }
          dre[(SP_TILE * wave + row) * SP_TILE + col] = 2.f * re[r] * g;
          dim[(SP_TILE * wave + row) * SP_TILE + col] = 2.f * im[r] * g;
        }
      }
      const int nkv = nk - ks * FR_WAVES < FR_WAVES ? nk - ks * FR_WAVES : FR_WAVES;   // row tiles held in dre / dim
      for (int ms = 0; ms * FR_WAVES < nk; ++ms) {
        // ---- G_I[m][t] = sum_k c dRe - s dIm,  G_Q[m][t] = sum_k s dRe + c dIm: one 32-sample segment per wave
        const int mi = ms * FR_WAVES + wave;
        const bool has_m = mi < nk;                             // wave-uniform
        f32x16 gi = {}, gq = {};
        for (int kk = 0; kk < nkv; ++kk) {
          __syncthreads();                                      // dre / dim written; G of the previous step gathered
          if (has_m)
            for (int q = lane; q < 512; q += IQ_WAVE) block_store(blk, q, block_load(a.table, n, mi, ks * FR_WAVES + kk, q));
          __syncthreads();
          if (has_m) {
#pragma unroll
            for (int s = 0; s < SP_TILE / 2; ++s) {
              const int kr = 2 * s + half;
              const float ac = blk[col * SP_TS + kr], as = blk[(SP_TILE + col) * SP_TS + kr];
              const float br = dre[(SP_TILE * kk + kr) * SP_TILE + col], bi = dim[(SP_TILE * kk + kr) * SP_TILE + col];
              gi = __builtin_amdgcn_mfma_f32_32x32x2f32(ac, br, gi, 0, 0, 0);
              gi = __builtin_amdgcn_mfma_f32_32x32x2f32(-as, bi, gi, 0, 0, 0);
              gq = __builtin_amdgcn_mfma_f32_32x32x2f32(as, br, gq, 0, 0, 0);
              gq = __builtin_amdgcn_mfma_f32_32x32x2f32(ac, bi, gq, 0, 0, 0);
            }
          }
        }
        if (has_m) {                                            // only this wave read its block: it may overwrite it
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int row = acc_row(r, half);
            blk[row * SP_TS + col] = gi[r];
            blk[(SP_TILE + row) * SP_TS + col] = gq[r];
          }
        }
        __syncthreads();
        // ---- overlap-add: sample j takes G[m][t] of every column t of the tile with m = j + pad - t*hop in this segment group
        const long mlo = (long)ms * FR_WAVES * SP_TILE;
        const long mhi = mlo + FR_WAVES * SP_TILE < n ? mlo + FR_WAVES * SP_TILE : (long)n;
        overlap_add<2>(dxi, dxq, blocks, SP_BLOCK, SP_TS, SP_TILE * SP_TS, t0, tcols, hop, pad, mlo, mhi, len, tid);
      }
    }
  }
}

// -> IQ_OK or the refusal; nothing is launched and no pointer dereferenced (other than par) before this returns IQ_OK
int check(const void* x, const void* table, const void* io_a, const void* io_b, int len, const iq_spectrogram_t* p) {
  if (!x || !table || !io_a || !io_b || !p) return IQ_ERR_ARG;
  if (len <= 0 || p->hop < 1 || p->width < 1 || p->pad < 0 || (p->mode & ~1)) return IQ_ERR_ARG;
  if (!is_finite(p->inv_norm) || !is_finite(p->floor) || !is_finite(p->scale) || !is_finite(p->shift)) return IQ_ERR_ARG;
  if (p->mode == 1 && !(p->floor > 0.f)) return IQ_ERR_ARG;
  if (((uintptr_t)x & 3) || ((uintptr_t)table & 15) || ((uintptr_t)io_a & 3) || ((uintptr_t)io_b & 3)) return IQ_ERR_ARG;
  if (!fft_size_ok(p->n_fft) || !frame_fits(len)) return IQ_ERR_UNSUPPORTED;
  return IQ_OK;
}

SpArgs pack(const float* x, const float* table, int len, const iq_spectrogram_t* p) {
  SpArgs a;
  a.x = x; a.table = table; a.out = nullptr; a.dout = nullptr; a.dx = nullptr; a.len = len; a.p = *p;
  a.vec4 = frame_vec4(x, len);
  return a;
}

}  // namespace

extern "C" int iq_frames_spectrogram(const float* x, const float* table, float* out, int n_frames, int len,
                                     const iq_spectrogram_t* par, iq_stream_t stream) {
  const int rc = check(x, table, out, out, len, par);
  if (rc != IQ_OK) return rc;
  if (n_frames <= 0) return IQ_OK;
  hipStream_t st = (hipStream_t)stream;
  IQ_PROF(IQ_FAM_MISC, st);
  SpArgs a = pack(x, table, len, par);
  a.out = out;
  const int n = par->n_fft;
  const size_t lds = ((size_t)frame_floats(len) + SP_BLOCK) * sizeof(float);
  const double cols = (double)n_frames * par->width;
  IQ_PROF_K((double)n_frames * len * 8 + cols * n * 4 + 8.0 * n * n, 8.0 * cols * n * n, "spectrogram_fwd_kernel");
  launch_frames(spectrogram_fwd_kernel, dim3(n_frames, n / SP_TILE), lds, st, a);
  return iq_launch_status();
}

extern "C" int iq_frames_spectrogram_bwd(const float* x, const float* table, const float* dout, float* dx, int n_frames, int len,
                                         const iq_spectrogram_t* par, iq_stream_t stream) {
  const int rc = check(x, table, dout, dx, len, par);
  if (rc != IQ_OK) return rc;
  if (n_frames <= 0) return IQ_OK;
  hipStream_t st = (hipStream_t)stream;
  IQ_PROF(IQ_FAM_MISC, st);
  SpArgs a = pack(x, table, len, par);
  a.dout = dout; a.dx = dx;
  const int n = par->n_fft;
  const size_t lds = ((size_t)frame_floats(len) + 2 * SP_DROWS * SP_TILE + FR_WAVES * SP_BLOCK) * sizeof(float);
  const double cols = (double)n_frames * par->width;
  IQ_PROF_K((double)n_frames * len * 16 + cols * n * 4 + 8.0 * n * n, 16.0 * cols * n * n, "spectrogram_bwd_kernel");
  launch_frames(spectrogram_bwd_kernel, n_frames, lds, st, a);
  return iq_launch_status();
}
