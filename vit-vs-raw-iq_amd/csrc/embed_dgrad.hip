// Data gradient of the embedding (gfx950): dsrc = unpatchify(demb . W_emb).
//
// Both embeddings are non-overlapping strided convolutions (Conv2d k = s = p for the ViT, Conv1d k = s for raw IQ), so a
// patch is a permutation of input elements: patchify_kernel (misc.hip) gathers them into rows of [B*tok, Kpad] and this
// kernel scatters the product rows back to where they came from.  Input elements that no patch covers get exactly 0.
//
//   demb   bf16 [B*tok, D]    gradient at the conv output (the workspace's demb, or a cast of the caller's fp32 gradient)
//   W      bf16 [D, Kpad]     the padded embedding weight (the plan's shadow at sh_embw); columns >= P are never stored
//   dsrc   fp32, the input's layout: (B, C, H, W) for kind 0, (B, C, L) for kind 1
//
// kind 1 is kind 0 with a 1 x p patch on a 1 x L image, so one address map serves both: token t of frame b starts at
// (row (t / gw) * ph, column (t % gw) * pw) of every channel plane, and product column n = (c, i, j) is channel c, row i,
// column j of the patch (the conv weight's [C, ph, pw] flattening).
//
// MFMA path (P > 16): mfma_f32_16x16x32_bf16, K = D in steps of 32.  The B operand runs along D, the strided direction of
// W, so every K step stages W[k0 .. k0+31][column chunk] into LDS transposed by the staging store (row = column n, 32 k
// plus 8 of padding, 80 B); a lane then reads its 8 consecutive k of column n with one ds_read_b128.  Workgroup = 8 waves
// x 16 rows = 128 rows of demb x one chunk of 16*NT columns (NT up to 16: 256 columns, 64 accumulator registers per lane);
// the column chunks of one row tile are adjacent block indices, so a demb tile read twice comes from L2.  W is restaged per
// K step (20 KB at NT 16), which keeps the LDS small for any D (ViT-Base: D 768, 384 KB of W would not fit in 160 KiB).
// VALU path (P <= 16, the raw-IQ conv1d embedding has P = 2): one row per thread, W as fp32 [D][P] in LDS read by broadcast.
// Blocks past the product tiles write the zeros of the uncovered border.  No atomics: two calls give the same bits.
#include "common.h"
#include "iqvit.h"
#include "prof.h"

namespace {

struct EdGeo {
  int C, H, W, ph, pw, gw, tok;   // image planes H x W (kind 1: 1 x L), patch ph x pw, gw patches per image row
  int Hc, Wc;                     // covered extent: (H / ph) * ph rows, (W / pw) * pw columns
};

constexpr int ED_WAVES = 8, ED_ROWS = 16 * ED_WAVES, ED_KS = 40;   // rows per workgroup, LDS row stride (bf16)

__device__ __forceinline__ long ed_row_off(const EdGeo& g, int m) {
  const int b = m / g.tok, t = m - (m / g.tok) * g.tok;
  const int gy = t / g.gw, gx = t - (t / g.gw) * g.gw;
  return ((long)b * g.C * g.H + (long)gy * g.ph) * g.W + (long)gx * g.pw;
}
__device__ __forceinline__ long ed_col_off(const EdGeo& g, int n) {
  const int pp = g.ph * g.pw;
  const int c = n / pp, rem = n - (n / pp) * pp;
  const int i = rem / g.pw, j = rem - (rem / g.pw) * g.pw;
  return ((long)c * g.H + i) * g.W + j;
}

// zeros where no patch reaches: per (frame, channel) plane, rows Hc .. H-1 (all columns), then columns Wc .. W-1 of rows < Hc
__device__ void ed_zero_border(const EdGeo& g, float* __restrict__ dsrc, long n_zero, long first, long stride) {
  const long U = (long)g.H * g.W - (long)g.Hc * g.Wc, band1 = (long)(g.H - g.Hc) * g.W;
  for (long id = first; id < n_zero; id += stride) {
    const long plane = id / U, u = id - plane * U;
    int h, w;
    if (u < band1) {
      h = g.Hc + (int)(u / g.W); w = (int)(u % g.W);
    } else {
      const long v = u - band1;
      const int wr = g.W - g.Wc;
      h = (int)(v / wr); w = g.Wc + (int)(v % wr);
    }
    dsrc[plane * g.H * g.W + (long)h * g.W + w] = 0.f;
  }
}

template <int NT>
__global__ __launch_bounds__(64 * ED_WAVES) void embed_dgrad_mfma_kernel(const bf16* __restrict__ demb, const bf16* __restrict__ Wt,
                                                                        int Kpad, float* __restrict__ dsrc, EdGeo g, int D, int MT,
                                                                        int P, int col_chunks, int tiles, long n_zero) {
  __shared__ bf16 ws[16 * NT * ED_KS];
  const int bid = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (bid >= tiles) {            // border blocks
    ed_zero_border(g, dsrc, n_zero, (long)(bid - tiles) * blockDim.x + tid, (long)(gridDim.x - tiles) * blockDim.x);
    return;
  }
  const int rt = bid / col_chunks, cc = bid - rt * col_chunks;
  const int n0 = cc * 16 * NT, row = rt * ED_ROWS + wave * 16 + (lane & 15), kl = 8 * (lane >> 4);
  f32x4 acc[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < D; k0 += 32) {
    // stage W[k0 .. k0+31][n0 .. n0+16NT) transposed: 8 columns of one k per 16 B load, 8 two-byte stores
    for (int v = tid; v < 32 * 2 * NT; v += 64 * ED_WAVES) {
      const int kk = v / (2 * NT), cv = v - kk * (2 * NT);
      const int k = k0 + kk, n = n0 + cv * 8;
      bf16x8 w = {};
      if (k < D && n < Kpad) w = *reinterpret_cast<const bf16x8*>(Wt + (long)k * Kpad + n);
#pragma unroll
      for (int e = 0; e < 8; ++e) ws[(cv * 8 + e) * ED_KS + kk] = w[e];
    }
    bf16x8 a = {};
    if (row < MT && k0 + kl < D) a = *reinterpret_cast<const bf16x8*>(demb + (long)row * D + k0 + kl);
    __syncthreads();
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const bf16x8 b = *reinterpret_cast<const bf16x8*>(ws + (j * 16 + (lane & 15)) * ED_KS + kl);
      acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc[j], 0, 0, 0);
    }
    __syncthreads();
  }
  // lane: column n0 + 16 j + (lane & 15), rows 4 (lane >> 4) + r of the wave's 16
  const int mb = rt * ED_ROWS + wave * 16 + 4 * (lane >> 4);
  long roff[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) roff[r] = mb + r < MT ? ed_row_off(g, mb + r) : -1;
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int n = n0 + j * 16 + (lane & 15);
    if (n >= P) continue;
    const long co = ed_col_off(g, n);
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (roff[r] >= 0) dsrc[roff[r] + co] = acc[j][r];
  }
}

template <int PT>
__global__ __launch_bounds__(256) void embed_dgrad_valu_kernel(const bf16* __restrict__ demb, const bf16* __restrict__ Wt, int Kpad,
                                                               float* __restrict__ dsrc, EdGeo g, int D, int MT, int P, int tiles,
                                                               long n_zero) {
  extern __shared__ float wf[];   // [D][PT]
  const int bid = blockIdx.x, tid = threadIdx.x;
  if (bid >= tiles) {
    ed_zero_border(g, dsrc, n_zero, (long)(bid - tiles) * blockDim.x + tid, (long)(gridDim.x - tiles) * blockDim.x);
    return;
  }
  for (int i = tid; i < D * PT; i += blockDim.x) {
    const int k = i / PT, n = i - (i / PT) * PT;
    wf[i] = n < P ? (float)Wt[(long)k * Kpad + n] : 0.f;
  }
  __syncthreads();
  const int m = bid * 256 + tid;
  if (m >= MT) return;
  float acc[PT];
#pragma unroll
  for (int n = 0; n < PT; ++n) acc[n] = 0.f;
  const bf16* rowp = demb + (long)m * D;
  for (int k = 0; k < D; k += 8) {
    float a[8];
    unpack8(*reinterpret_cast<const bf16x8*>(rowp + k), a);
#pragma unroll
    for (int e = 0; e < 8; ++e)
#pragma unroll
      for (int n = 0; n < PT; ++n) acc[n] += a[e] * wf[(k + e) * PT + n];
  }
  const long ro = ed_row_off(g, m);
#pragma unroll
  for (int n = 0; n < PT; ++n)
    if (n < P) dsrc[ro + ed_col_off(g, n)] = acc[n];
}

int zero_blocks(long n_zero) {
  if (n_zero <= 0) return 0;
  long b = (n_zero + 255) / 256;
  return (int)(b < 512 ? b : 512);
}

}  // namespace

extern "C" int iq_embed_dgrad(const void* demb, const void* w_bf16, int Kpad, float* dsrc, int kind, int B, int C, int H, int W,
                              int p, int D, iq_stream_t stream) {
  if (!demb || !w_bf16 || !dsrc) return IQ_ERR_ARG;
  if (B < 0 || C <= 0 || H <= 0 || p <= 0 || D <= 0 || (D % 8) || Kpad <= 0 || (Kpad % 8)) return IQ_ERR_ARG;
  if (((uintptr_t)demb | (uintptr_t)w_bf16) & 15) return IQ_ERR_ARG;
  EdGeo g;
  g.C = C;
  if (kind == 0) {
    if (W <= 0) return IQ_ERR_ARG;
    g.H = H; g.W = W; g.ph = p; g.pw = p;
  } else if (kind == 1) {
    g.H = 1; g.W = H; g.ph = 1; g.pw = p;        // (B, C, L): H carries L, as in iq_patchify
  } else {
    return IQ_ERR_ARG;
  }
  g.gw = g.W / g.pw;
  g.tok = (g.H / g.ph) * g.gw;
  g.Hc = (g.H / g.ph) * g.ph; g.Wc = g.gw * g.pw;
  const int P = C * g.ph * g.pw;
  if (g.tok <= 0 || Kpad < P) return IQ_ERR_ARG;
  if (B == 0) return IQ_OK;
  if ((long)B * g.tok > 0x7fffffffL) return IQ_ERR_UNSUPPORTED;
  IQ_PROF(IQ_FAM_MISC, stream);
  hipStream_t st = (hipStream_t)stream;
  const int MT = B * g.tok;
  const long n_zero = (long)B * C * ((long)g.H * g.W - (long)g.Hc * g.Wc);
  const int zb = zero_blocks(n_zero);
  const double bytes = (double)MT * D * 2 + (double)D * Kpad * 2 + (double)B * C * g.H * g.W * 4;
  const bf16* a = (const bf16*)demb;
  const bf16* w = (const bf16*)w_bf16;
  if (P <= 16) {
    const int tiles = (MT + 255) / 256;
    const size_t lds = (size_t)D * (P <= 2 ? 2 : P <= 4 ? 4 : P <= 8 ? 8 : 16) * sizeof(float);
    if (lds > 64 * 1024) return IQ_ERR_UNSUPPORTED;
#define ED_VALU(PT)                                                                                               \
  do {                                                                                                            \
    IQ_PROF_K(bytes, 2.0 * MT * D * P, "embed_dgrad_valu_kernel<%d>", PT);                                        \
    embed_dgrad_valu_kernel<PT><<<tiles + zb, 256, lds, st>>>(a, w, Kpad, dsrc, g, D, MT, P, tiles, n_zero);      \
  } while (0)
    if (P <= 2) ED_VALU(2);
    else if (P <= 4) ED_VALU(4);
    else if (P <= 8) ED_VALU(8);
    else ED_VALU(16);
#undef ED_VALU
    return iq_launch_status();
  }
  const int need = (P + 15) / 16;
  const int NT = need <= 2 ? 2 : need <= 4 ? 4 : need <= 8 ? 8 : 16;
  const int col_chunks = (need + NT - 1) / NT;
  const long tiles_l = (long)((MT + ED_ROWS - 1) / ED_ROWS) * col_chunks;
  if (tiles_l + zb > 0x7fffffffL) return IQ_ERR_UNSUPPORTED;
  const int tiles = (int)tiles_l;
#define ED_MFMA(NT_)                                                                                              \
  do {                                                                                                            \
    IQ_PROF_K(bytes, 2.0 * MT * D * P, "embed_dgrad_mfma_kernel<%d>", NT_);                                       \
    embed_dgrad_mfma_kernel<NT_><<<tiles + zb, 64 * ED_WAVES, 0, st>>>(a, w, Kpad, dsrc, g, D, MT, P, col_chunks, tiles, n_zero); \
  } while (0)
  if (NT == 2) ED_MFMA(2);
  else if (NT == 4) ED_MFMA(4);
  else if (NT == 8) ED_MFMA(8);
  else ED_MFMA(16);
#undef ED_MFMA
  return iq_launch_status();
}
