// Attention probabilities and attention rollout, read back from what a forward left in its workspace, for gfx950 (MI355X).
//
// Reference: MultiHeadAttention.forward receives the attention matrix from ScaleDotProductAttention and drops it
// (V/models/layers/multi_head_attention.py:24,30, "5. visualize attention map"); scale_dot_product_attention.py:23-39 forms
// it as softmax(q k^T / sqrt(dh)).  The fused forward (attention.hip) never writes that matrix.  It keeps the packed bf16
// q|k|v and the fp32 log-sum-exp of every query row, and these kernels rebuild
//   P[q, key] = exp2(q.k * log2(e)/sqrt(dh) - lse[q] * log2(e))
// from them: the forward's products (mfma_f32_16x16x32_bf16, key tile as A, query tile as B, the same contraction slots) and
// the backward's exponent argument (attention.hip, attn_bwd_kernel / attn_frame_bwd_kernel).
//
// Work unit: one head's 32-query block against a chunk of up to KC = 256 keys.  The Q block and the K chunk are staged in LDS;
// wave w computes key tiles w and w + 8 (16 keys each) for both 16-query halves, so the lane of query c16 holds 4 consecutive
// keys, which go to an fp32 LDS tile Pt[32][KC].  From there:
//   rows 0, heads 0   the tile is copied out.  Its rows are consecutive in `out` (one contiguous range when the chunk is the
//                     whole row): 16-byte stores from the first 16-byte boundary on, 4-byte stores at the two ragged ends
//                     (S is odd wherever a CLS token precedes a power-of-two token count)
//   rows 0, heads 1   the lanes sum their tiles over the heads in registers (h = 0 .. H-1), scale by 1/H, then as above
//   rows 1, 2         thread `col` sums its key column of the tile (query 0 only, resp. every real query, in order)
// No atomics: every output element is written by one thread of one workgroup and every sum runs in a fixed order, so two
// calls give the same bits.
//
// Gradient-weighted maps and the relevance step (Chefer, Gur & Wolf, ICCV 2021, arXiv 2103.15679, eqs. 5-6) take the gradient
// dO of the concatenated attention-core output as well: dP[q, key] = dO_h[q].v_h[key] is a second mfma_f32_16x16x32_bf16 product
// of the same tile shape (V chunk as A, dO block as B), and G = P * dP (clamped at 0 per head when asked) replaces P above.
// The relevance step r_out = r_in + r_in * mean_h max(G_h, 0) runs one workgroup per (frame, block of 128 keys): wave w owns
// key tile w, its lanes accumulate r_in[q] * max(G, 0) over heads and query tiles in registers and the 16 query lanes of a
// key are reduced by a fixed butterfly at the end.
#include <stdint.h>

#include "attn_common.h"
#include "attn_maps.h"
#include "iqvit.h"
#include "prof.h"

namespace {

constexpr int PM_THREADS = 512;
constexpr int PM_WAVES = PM_THREADS / 64;
constexpr int QB = 32;                       // queries per block
constexpr int KC = 256;                      // keys per chunk
constexpr int KTW = KC / 16 / PM_WAVES;      // key tiles per wave
constexpr int PLD = KC + 4;                  // fp32 row stride of the probability tile

// rows [r0, r0 + nrows) of a head slice (global row stride ldg) -> LDS image; rows >= S are zero
template <int DH>
__device__ __forceinline__ void stage(bf16* img, const bf16* base, long ldg, int r0, int nrows, int S, int tid) {
  constexpr int CPR = AttCfg<DH>::CPR, LD = AttCfg<DH>::LD;
  for (int id = tid; id < nrows * CPR; id += PM_THREADS) {
    const int r = id / CPR, c = id - r * CPR;
    bf16x8 v = {};
    if (r0 + r < S) v = *reinterpret_cast<const bf16x8*>(base + (long)(r0 + r) * ldg + c * 8);
    *reinterpret_cast<bf16x8*>(img + r * LD + c * 8) = v;
  }
}

// P^T tiles of this wave: p[u][j] = key tile (wave + 8 j) x query half u.  Lane: query c16 of the half, keys 4g .. 4g+3 of the
// tile.  lq[u]: the lane's query lse * log2(e).  Keys >= S give 0; tiles past the chunk are not computed.
template <int DH>
__device__ __forceinline__ void tile_probs(const bf16* Qs, const bf16* Ks, const float lq[2], bool u1, int kc, int k0, int S,
                                           float scale_log2, int wave, int lane, f32x4 p[2][KTW]) {
  constexpr int KS = AttCfg<DH>::KS;
  const int c16 = lane & 15, g = lane >> 4;
  bf16x8 qf[2][KS];
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int s = 0; s < KS; ++s) qf[u][s] = row_frag<DH>(Qs, HeadRows<DH>{}, u * 16 + c16, s, lane);
#pragma unroll
  for (int j = 0; j < KTW; ++j) {
    const int kt = wave + PM_WAVES * j;
    p[0][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    p[1][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (kt * 16 >= kc) continue;                 // wave-uniform
    bf16x8 kf[KS];
#pragma unroll
    for (int s = 0; s < KS; ++s) kf[s] = row_frag<DH>(Ks, HeadRows<DH>{}, kt * 16 + c16, s, lane);
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      if (u == 1 && !u1) continue;               // wave-uniform: the second half holds no query
      f32x4 a = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < KS; ++s) a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[s], qf[u][s], a, 0, 0, 0);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float pv = fast_exp2(a[r] * scale_log2 - lq[u]);
        p[u][j][r] = k0 + kt * 16 + 4 * g + r < S ? pv : 0.f;
      }
    }
  }
}

__device__ __forceinline__ void tile_to_lds(float* Pt, const f32x4 p[2][KTW], int kc, int wave, int lane) {
  const int c16 = lane & 15, g = lane >> 4;
#pragma unroll
  for (int j = 0; j < KTW; ++j) {
    const int kt = wave + PM_WAVES * j;
    if (kt * 16 >= kc) continue;
#pragma unroll
    for (int u = 0; u < 2; ++u) *reinterpret_cast<f32x4*>(Pt + (u * 16 + c16) * PLD + kt * 16 + 4 * g) = p[u][j];
  }
}

// dst[0 .. n) <- tile rows of kc elements read in order (element e = row e / kc, column e % kc); threads t of nt.
// 16-byte stores from dst's first 16-byte boundary on, 4-byte stores for at most 3 elements at either end.
__device__ __forceinline__ void flush_rows(float* dst, int n, int kc, const float* Pt, int t, int nt) {
  const int lead = min((int)((0u - (unsigned)((uintptr_t)dst >> 2)) & 3u), n);
  const int nq4 = (n - lead) >> 2;
  if (t < lead) {
    const int r = t / kc;
    dst[t] = Pt[r * PLD + t - r * kc];
  }
  for (int i = t; i < nq4; i += nt) {
    const int e = lead + 4 * i;
    int r = e / kc, c = e - r * kc;
    f32x4 v;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      v[j] = Pt[r * PLD + c];
      if (++c == kc) { c = 0; ++r; }
    }
    *reinterpret_cast<f32x4*>(dst + e) = v;
  }
  const int e = lead + 4 * nq4 + t;
  if (e < n) {
    const int r = e / kc;
    dst[e] = Pt[r * PLD + e - r * kc];
  }
}

struct ProbsArgs {
  const bf16* qkv;
  const float* lse;
  float* out;
  long bstride;
  int S, H, rows, heads;
  int nhg, nqg;        // head groups / query-block groups per frame in the grid (1: the workgroup loops over all of them)
  float scale_log2;
  const bf16* dout;    // attn_grad_probs_kernel only: dO [B*S, H*dh] and whether G is clamped at 0
  int positive;
};

// The raw products of this wave's tiles in the layout of tile_probs: d[u][j] = A tile (wave + 8 j) x B half u.
template <int DH>
__device__ __forceinline__ void tile_dots(const bf16* Bs, const bf16* As, bool u1, int kc, int wave, int lane, f32x4 d[2][KTW]) {
  constexpr int KS = AttCfg<DH>::KS;
  const int c16 = lane & 15;
  bf16x8 bf[2][KS];
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int s = 0; s < KS; ++s) bf[u][s] = row_frag<DH>(Bs, HeadRows<DH>{}, u * 16 + c16, s, lane);
#pragma unroll
  for (int j = 0; j < KTW; ++j) {
    const int kt = wave + PM_WAVES * j;
    d[0][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    d[1][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (kt * 16 >= kc) continue;
    bf16x8 af[KS];
#pragma unroll
    for (int s = 0; s < KS; ++s) af[s] = row_frag<DH>(As, HeadRows<DH>{}, kt * 16 + c16, s, lane);
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      if (u == 1 && !u1) continue;
#pragma unroll
      for (int s = 0; s < KS; ++s) d[u][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[s], bf[u][s], d[u][j], 0, 0, 0);
    }
  }
}

// GRAD = false: P (attn_probs_kernel).  GRAD = true: G = P * dP, max(G, 0) when a.positive (attn_grad_probs_kernel): after P,
// the dO block and the V chunk are staged where Q and K were and dP is formed in the same layout.
template <int DH, bool GRAD>
__device__ __forceinline__ void probs_body(const ProbsArgs& a) {
  using Cf = AttCfg<DH>;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  bf16* Qs = reinterpret_cast<bf16*>(smem);
  bf16* Ks = Qs + QB * Cf::LD;
  float* Pt = reinterpret_cast<float*>(Ks + KC * Cf::LD);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c16 = lane & 15;
  const int S = a.S, H = a.H, D = H * DH;
  const long ldg = 3L * D;
  const int nqb = a.rows == 1 ? 1 : (S + QB - 1) / QB;
  int wg = blockIdx.x;
  const int qg = wg % a.nqg;
  wg /= a.nqg;
  const int hg = wg % a.nhg, b = wg / a.nhg;
  const int h_lo = a.nhg == 1 ? 0 : hg, nh = a.nhg == 1 ? H : 1;
  const int qb_lo = a.nqg == 1 ? 0 : qg, nq = a.nqg == 1 ? nqb : 1;
  const bf16* fq = a.qkv + (long)b * S * ldg;
  float* ob = a.out + (long)b * a.bstride;
  const bool qouter = a.rows == 0;     // rows 0: heads innermost (their mean accumulates in registers); 1, 2: queries innermost
  f32x4 acc[2][KTW];
#pragma unroll
  for (int j = 0; j < KTW; ++j) { acc[0][j] = f32x4{0.f, 0.f, 0.f, 0.f}; acc[1][j] = f32x4{0.f, 0.f, 0.f, 0.f}; }
  float csum = 0.f;
  for (int k0 = 0; k0 < S; k0 += KC) {
    const int kc = min(KC, S - k0);
    for (int t = 0; t < nh * nq; ++t) {
      const int hi = qouter ? t % nh : t / nq, qi = qouter ? t / nh : t % nq;
      const int h = h_lo + hi, q0 = (qb_lo + qi) * QB;
      const bf16* hq = fq + h * DH;
      stage<DH>(Qs, hq, ldg, q0, QB, S, tid);
      stage<DH>(Ks, hq + D, ldg, k0, (kc + 15) / 16 * 16, S, tid);
      float lq[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int q = q0 + u * 16 + c16;
        lq[u] = q < S ? a.lse[((long)b * H + h) * S + q] * LOG2E : 0.f;
      }
      __syncthreads();
      f32x4 p[2][KTW];
      tile_probs<DH>(Qs, Ks, lq, a.rows != 1 && q0 + 16 < S, kc, k0, S, a.scale_log2, wave, lane, p);
      __syncthreads();                           // Qs / Ks free for the next item
      if (GRAD) {
        stage<DH>(Qs, a.dout + (long)b * S * D + h * DH, D, q0, QB, S, tid);
        stage<DH>(Ks, hq + 2 * D, ldg, k0, (kc + 15) / 16 * 16, S, tid);
        __syncthreads();
        f32x4 dp[2][KTW];
        tile_dots<DH>(Qs, Ks, a.rows != 1 && q0 + 16 < S, kc, wave, lane, dp);
        __syncthreads();
#pragma unroll
        for (int j = 0; j < KTW; ++j)
#pragma unroll
          for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const float g = p[u][j][r] * dp[u][j][r];    // keys >= S: p is 0; queries >= S are never read
              p[u][j][r] = a.positive ? fmaxf(g, 0.f) : g;
            }
      }
      const int nrow = a.rows == 1 ? 1 : min(QB, S - q0);
      if (a.rows == 0 && a.heads == 1) {
        const float inv = 1.0f / H;
#pragma unroll
        for (int j = 0; j < KTW; ++j)
#pragma unroll
          for (int u = 0; u < 2; ++u) acc[u][j] += p[u][j];
        if (hi < nh - 1) continue;
#pragma unroll
        for (int j = 0; j < KTW; ++j)
#pragma unroll
          for (int u = 0; u < 2; ++u) { p[u][j] = acc[u][j] * inv; acc[u][j] = f32x4{0.f, 0.f, 0.f, 0.f}; }
      }
      tile_to_lds(Pt, p, kc, wave, lane);
      __syncthreads();
      // (the next write of Pt follows the next item's two barriers)
      if (a.rows == 0) {
        float* dst = ob + ((long)(a.heads ? 0 : h) * S + q0) * S;
        if (kc == S) flush_rows(dst, nrow * S, S, Pt, tid, PM_THREADS);
        else
          for (int r = wave; r < nrow; r += PM_WAVES) flush_rows(dst + (long)r * S + k0, kc, kc, Pt + r * PLD, lane, 64);
      } else if (tid < kc) {
        float s = 0.f;
        for (int r = 0; r < nrow; ++r) s += Pt[r * PLD + tid];
        csum += s;
        if (a.heads ? t == nh * nq - 1 : qi == nq - 1) {
          const float norm = (a.rows == 2 ? 1.0f / S : 1.0f) * (a.heads ? 1.0f / H : 1.0f);
          ob[(long)(a.heads ? 0 : h) * S + k0 + tid] = csum * norm;
          csum = 0.f;
        }
      }
    }
  }
}

template <int DH>
__global__ __launch_bounds__(PM_THREADS) void attn_probs_kernel(ProbsArgs a) { probs_body<DH, false>(a); }

template <int DH>
__global__ __launch_bounds__(PM_THREADS) void attn_grad_probs_kernel(ProbsArgs a) { probs_body<DH, true>(a); }

// Rollout: one workgroup per frame, r and the next r in LDS.  Per layer (top down), chunk of keys, head and query block, the
// P tile goes to LDS and thread `col` adds sum_q r[q] P[q, col] in order; the chunk's new r is
// alpha * (that / H) + (1 - alpha) * r[col].
struct RolloutArgs {
  const unsigned char* qkv0;
  long qkv_lstride;
  const unsigned char* lse0;
  long lse_lstride;
  float* out;
  int L, S, H, cls;
  float alpha, scale_log2;
};

template <int DH>
__global__ __launch_bounds__(PM_THREADS) void attn_rollout_kernel(RolloutArgs a) {
  using Cf = AttCfg<DH>;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  bf16* Qs = reinterpret_cast<bf16*>(smem);
  bf16* Ks = Qs + QB * Cf::LD;
  float* Pt = reinterpret_cast<float*>(Ks + KC * Cf::LD);
  const int S = a.S, H = a.H, D = H * DH;
  const int spad = (S + QB - 1) / QB * QB;
  float* r = Pt + QB * PLD;
  float* rn = r + spad;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c16 = lane & 15;
  const long ldg = 3L * D;
  const int b = blockIdx.x, nqb = spad / QB;
  for (int i = tid; i < spad; i += PM_THREADS) r[i] = i < S ? (a.cls ? (i == 0 ? 1.f : 0.f) : 1.0f / S) : 0.f;
  __syncthreads();
  for (int l = a.L - 1; l >= 0; --l) {
    const bf16* fq = reinterpret_cast<const bf16*>(a.qkv0 + l * a.qkv_lstride) + (long)b * S * ldg;
    const float* lse = reinterpret_cast<const float*>(a.lse0 + l * a.lse_lstride) + (long)b * H * S;
    for (int k0 = 0; k0 < S; k0 += KC) {
      const int kc = min(KC, S - k0);
      float col = 0.f;
      for (int t = 0; t < H * nqb; ++t) {
        const int h = t / nqb, q0 = (t - h * nqb) * QB;
        const bf16* hq = fq + h * DH;
        stage<DH>(Qs, hq, ldg, q0, QB, S, tid);
        stage<DH>(Ks, hq + D, ldg, k0, (kc + 15) / 16 * 16, S, tid);
        float lq[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const int q = q0 + u * 16 + c16;
          lq[u] = q < S ? lse[(long)h * S + q] * LOG2E : 0.f;
        }
        __syncthreads();
        f32x4 p[2][KTW];
        tile_probs<DH>(Qs, Ks, lq, q0 + 16 < S, kc, k0, S, a.scale_log2, wave, lane, p);
        __syncthreads();
        tile_to_lds(Pt, p, kc, wave, lane);
        __syncthreads();
        if (tid < kc) {
          const int nrow = min(QB, S - q0);
          float s = 0.f;
          for (int i = 0; i < nrow; ++i) s += r[q0 + i] * Pt[i * PLD + tid];
          col += s;
        }
      }
      if (tid < kc) rn[k0 + tid] = a.alpha * (col * (1.0f / H)) + (1.0f - a.alpha) * r[k0 + tid];
    }
    __syncthreads();
    float* tmp = r;
    r = rn;
    rn = tmp;
  }
  for (int i = tid; i < S; i += PM_THREADS) a.out[(long)b * S + i] = r[i];
}

// Relevance step: one workgroup per (frame, block of RKB keys).  Per head the K and V rows of the block are staged once; per
// chunk of RQC queries the Q and dO rows.  Wave w holds key tile w (its K and V fragments in registers for the head) and runs
// both products against each 16-query tile of the chunk; lane (c16, g) accumulates r_in[q] * max(P * dP, 0) for query c16 and
// keys 4g .. 4g+3.  start 1 | 2: r_in is e_0 | 1/S (not read); with e_0 only query 0 contributes.
constexpr int RKB = PM_WAVES * 16;   // keys per workgroup
constexpr int RQC = 64;              // queries per staged chunk

struct StepArgs {
  const bf16* qkv;
  const float* lse;
  const bf16* dout;
  const float* rin;
  float* rout;
  int S, H, nkb, start;
  float scale_log2;
};

template <int DH>
__global__ __launch_bounds__(PM_THREADS) void attn_relevance_step_kernel(StepArgs a) {
  using Cf = AttCfg<DH>;
  constexpr int KS = Cf::KS;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  bf16* Ks = reinterpret_cast<bf16*>(smem);
  bf16* Vs = Ks + RKB * Cf::LD;
  bf16* Qs = Vs + RKB * Cf::LD;
  bf16* Ds = Qs + RQC * Cf::LD;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c16 = lane & 15, g = lane >> 4;
  const int S = a.S, H = a.H, D = H * DH;
  const long ldg = 3L * D;
  const int b = blockIdx.x / a.nkb, k0 = (blockIdx.x - b * a.nkb) * RKB;
  const int kc = min(RKB, S - k0);
  const bool live = wave * 16 < kc;              // wave-uniform: this wave's key tile holds a key
  const int qend = a.start == 1 ? 1 : S;         // r_in = e_0: query 0 alone
  const bf16* fq = a.qkv + (long)b * S * ldg;
  const bf16* fd = a.dout + (long)b * S * D;
  const float* lse = a.lse + (long)b * H * S;
  const float* rin = a.rin + (long)b * S;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int h = 0; h < H; ++h) {
    const bf16* hq = fq + h * DH;
    bf16x8 kf[KS], vf[KS];
    for (int q0 = 0; q0 < qend; q0 += RQC) {
      if (q0 == 0) {
        stage<DH>(Ks, hq + D, ldg, k0, RKB, S, tid);
        stage<DH>(Vs, hq + 2 * D, ldg, k0, RKB, S, tid);
      }
      stage<DH>(Qs, hq, ldg, q0, RQC, S, tid);
      stage<DH>(Ds, fd + h * DH, D, q0, RQC, S, tid);
      __syncthreads();
      if (live) {
        if (q0 == 0) {
#pragma unroll
          for (int s = 0; s < KS; ++s) {
            kf[s] = row_frag<DH>(Ks, HeadRows<DH>{}, wave * 16 + c16, s, lane);
            vf[s] = row_frag<DH>(Vs, HeadRows<DH>{}, wave * 16 + c16, s, lane);
          }
        }
#pragma unroll
        for (int u = 0; u < RQC / 16; ++u) {
          if (q0 + u * 16 >= qend) break;         // wave-uniform
          const int q = q0 + u * 16 + c16;
          const bool qv = q < qend;
          const float lq = qv ? lse[(long)h * S + q] * LOG2E : 0.f;
          const float rq = !qv ? 0.f : a.start == 0 ? rin[q] : a.start == 1 ? 1.f : 1.0f / S;
          f32x4 sc = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int s = 0; s < KS; ++s) {
            const bf16x8 qf = row_frag<DH>(Qs, HeadRows<DH>{}, u * 16 + c16, s, lane);
            const bf16x8 df = row_frag<DH>(Ds, HeadRows<DH>{}, u * 16 + c16, s, lane);
            sc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[s], qf, sc, 0, 0, 0);
            dp = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf[s], df, dp, 0, 0, 0);
          }
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float p = fast_exp2(sc[r] * a.scale_log2 - lq);
            const float gv = k0 + wave * 16 + 4 * g + r < S && qv ? fmaxf(p * dp[r], 0.f) : 0.f;
            acc[r] += rq * gv;
          }
        }
      }
      __syncthreads();                           // Qs / Ds (and at the next head Ks / Vs) free
    }
  }
  // sum over the 16 query lanes of each key (fixed butterfly), then r_out = r_in + acc / H
#pragma unroll
  for (int m = 1; m < 16; m <<= 1)
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[r] += __shfl_xor(acc[r], m);
  if (live && c16 == 0) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int k = k0 + wave * 16 + 4 * g + r;
      if (k < S) {
        const float rk = a.start == 0 ? rin[k] : a.start == 1 ? (k == 0 ? 1.f : 0.f) : 1.0f / S;
        a.rout[(long)b * S + k] = rk + acc[r] * (1.0f / H);
      }
    }
  }
}

template <int DH> constexpr size_t probs_lds() {
  return (size_t)QB * AttCfg<DH>::LD * 2 + (size_t)KC * AttCfg<DH>::LD * 2 + (size_t)QB * PLD * 4;
}

template <int DH, bool GRAD>
int launch_probs(const ProbsArgs& a, int B, hipStream_t st) {
  // per frame where the forward runs its per-frame kernel (short sequences); else per (frame, head, query block), with the
  // groups a fixed-order mean needs kept inside one workgroup
  const bool frame = a.S <= 128;
  ProbsArgs g = a;
  const int nqb = (a.S + QB - 1) / QB;
  if (a.rows == 0) {
    g.nhg = (a.heads == 1 || frame) ? 1 : a.H;
    g.nqg = frame ? 1 : nqb;
  } else {
    g.nhg = (a.heads == 1 || frame) ? 1 : a.H;
    g.nqg = 1;
  }
  const unsigned grid = (unsigned)((long)B * g.nhg * g.nqg);
  return launch_lds(GRAD ? attn_grad_probs_kernel<DH> : attn_probs_kernel<DH>, grid, PM_THREADS, probs_lds<DH>(), st, g);
}

template <int DH>
int launch_step(const StepArgs& a, int B, hipStream_t st) {
  return launch_lds(attn_relevance_step_kernel<DH>, (unsigned)((long)B * a.nkb), PM_THREADS,
                    (size_t)(2 * RKB + 2 * RQC) * AttCfg<DH>::LD * 2, st, a);
}

template <int DH>
int launch_rollout(const RolloutArgs& a, int B, hipStream_t st) {
  return launch_lds(attn_rollout_kernel<DH>, B, PM_THREADS, probs_lds<DH>() + (size_t)2 * padded32(a.S) * 4, st, a);
}

}  // namespace

extern "C" int iq_attn_probs(const void* qkv, const float* lse, float* out, long out_bstride, int B, int S, int H, int dh,
                             int rows, int heads, iq_stream_t stream) {
  if (B < 0 || H <= 0 || rows < 0 || rows > 2 || heads < 0 || heads > 1) return IQ_ERR_ARG;
  if (!iq_attn_supported(S, dh)) return IQ_ERR_UNSUPPORTED;
  if (B == 0) return IQ_OK;
  if (!qkv || !lse || !out || ((uintptr_t)qkv & 15) || ((uintptr_t)out & 3)) return IQ_ERR_ARG;
  if (out_bstride < (long)(heads ? 1 : H) * S * (rows == 0 ? S : 1)) return IQ_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  IQ_PROF(IQ_FAM_MISC, st);
  {
    const double qrows = rows == 1 ? 1.0 : (double)S;
    const double outb = 4.0 * B * (heads ? 1 : H) * (rows == 0 ? (double)S * S : (double)S);
    IQ_PROF_K(2.0 * B * S * 2.0 * H * dh + 4.0 * B * H * S + outb, 2.0 * B * H * qrows * S * dh, "attn_probs_kernel<%d>", dh);
  }
  ProbsArgs a;
  a.qkv = (const bf16*)qkv; a.lse = lse; a.out = out; a.bstride = out_bstride;
  a.S = S; a.H = H; a.rows = rows; a.heads = heads; a.nhg = 1; a.nqg = 1;
  a.scale_log2 = LOG2E / sqrtf((float)dh);
  a.dout = nullptr; a.positive = 0;
  return dispatch_dh(dh, [&](auto d) { return launch_probs<d(), false>(a, B, st); });
}

extern "C" int iq_attn_grad_probs(const void* qkv, const float* lse, const void* dout, float* out, long out_bstride, int B, int S,
                                  int H, int dh, int rows, int heads, int positive, iq_stream_t stream) {
  if (B < 0 || H <= 0 || rows < 0 || rows > 2 || heads < 0 || heads > 1 || positive < 0 || positive > 1) return IQ_ERR_ARG;
  if (!iq_attn_supported(S, dh)) return IQ_ERR_UNSUPPORTED;
  if (B == 0) return IQ_OK;
  if (!qkv || !lse || !dout || !out || ((uintptr_t)qkv & 15) || ((uintptr_t)dout & 15) || ((uintptr_t)out & 3)) return IQ_ERR_ARG;
  if (out_bstride < (long)(heads ? 1 : H) * S * (rows == 0 ? S : 1)) return IQ_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  IQ_PROF(IQ_FAM_MISC, st);
  {
    const double qrows = rows == 1 ? 1.0 : (double)S;
    const double outb = 4.0 * B * (heads ? 1 : H) * (rows == 0 ? (double)S * S : (double)S);
    IQ_PROF_K(2.0 * B * S * 3.0 * H * dh + 2.0 * B * qrows * H * dh + 4.0 * B * H * S + outb, 4.0 * B * H * qrows * S * dh,
              "attn_grad_probs_kernel<%d>", dh);
  }
  ProbsArgs a;
  a.qkv = (const bf16*)qkv; a.lse = lse; a.out = out; a.bstride = out_bstride;
  a.S = S; a.H = H; a.rows = rows; a.heads = heads; a.nhg = 1; a.nqg = 1;
  a.scale_log2 = LOG2E / sqrtf((float)dh);
  a.dout = (const bf16*)dout; a.positive = positive;
  return dispatch_dh(dh, [&](auto d) { return launch_probs<d(), true>(a, B, st); });
}

int attn_relevance_step_launch(const void* qkv, const float* lse, const void* dout, const float* r_in, float* r_out, int B, int S,
                               int H, int dh, int start, hipStream_t st) {
  if (B <= 0) return IQ_OK;
  if (!iq_attn_supported(S, dh)) return IQ_ERR_UNSUPPORTED;
  IQ_PROF(IQ_FAM_MISC, st);
  {
    const double qrows = start == 1 ? 1.0 : (double)S;
    IQ_PROF_K(2.0 * B * S * 3.0 * H * dh + 2.0 * B * qrows * H * dh + 4.0 * B * H * qrows + 4.0 * B * (qrows + 2.0 * S),
              4.0 * B * H * qrows * S * dh, "attn_relevance_step_kernel<%d>", dh);
  }
  StepArgs a;
  a.qkv = (const bf16*)qkv; a.lse = lse; a.dout = (const bf16*)dout; a.rin = r_in; a.rout = r_out;
  a.S = S; a.H = H; a.nkb = (S + RKB - 1) / RKB; a.start = start;
  a.scale_log2 = LOG2E / sqrtf((float)dh);
  return dispatch_dh(dh, [&](auto d) { return launch_step<d()>(a, B, st); });
}

extern "C" int iq_attn_relevance_step(const void* qkv, const float* lse, const void* dout, const float* r_in, float* r_out, int B,
                                      int S, int H, int dh, iq_stream_t stream) {
  if (B < 0 || H <= 0) return IQ_ERR_ARG;
  if (!iq_attn_supported(S, dh)) return IQ_ERR_UNSUPPORTED;
  if (B == 0) return IQ_OK;
  if (!qkv || !lse || !dout || !r_in || !r_out || ((uintptr_t)qkv & 15) || ((uintptr_t)dout & 15) || ((uintptr_t)r_in & 3) ||
      ((uintptr_t)r_out & 3))
    return IQ_ERR_ARG;
  const uintptr_t n = (uintptr_t)B * S * 4, i = (uintptr_t)r_in, o = (uintptr_t)r_out;
  if (i < o + n && o < i + n) return IQ_ERR_ARG;          // r_out is written while other workgroups still read r_in
  return attn_relevance_step_launch(qkv, lse, dout, r_in, r_out, B, S, H, dh, 0, (hipStream_t)stream);
}

int attn_rollout_launch(const unsigned char* qkv0, long qkv_lstride, const unsigned char* lse0, long lse_lstride, int L,
                        float* out, int B, int S, int H, int dh, int cls, float alpha, hipStream_t st) {
  if (B <= 0) return IQ_OK;
  if (!iq_attn_supported(S, dh)) return IQ_ERR_UNSUPPORTED;
  IQ_PROF(IQ_FAM_MISC, st);
  IQ_PROF_K((double)L * (2.0 * B * S * 2.0 * H * dh + 4.0 * B * H * S) + 4.0 * B * S, 2.0 * L * B * H * (double)S * S * (dh + 1),
            "attn_rollout_kernel<%d>", dh);
  RolloutArgs a;
  a.qkv0 = qkv0; a.qkv_lstride = qkv_lstride; a.lse0 = lse0; a.lse_lstride = lse_lstride; a.out = out;
  a.L = L; a.S = S; a.H = H; a.cls = cls; a.alpha = alpha; a.scale_log2 = LOG2E / sqrtf((float)dh);
  return dispatch_dh(dh, [&](auto d) { return launch_rollout<d()>(a, B, st); });
}
