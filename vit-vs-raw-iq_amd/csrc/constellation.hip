// Constellation front end (iq_frames_constellation / _bwd, include/iqvit.h): the smoothed 2-D density of the (I, Q) points of a
// planar (2, len) frame as a (height, width) image, with the power / log epilogue fused, and its adjoint.  With a separable
// profile the image is a Gram matrix over the points, D[r][c] = sum_n a[n][r] b[n][c], a from Q (rows), b from I (columns).
//
// Arithmetic: the fp32-input MFMA v_mfma_f32_32x32x2_f32 -- bit for bit an n-ordered fp32 fmaf chain.  Orientation: A[i = row]
// [k = point], B[k = point][j = column]; the accumulator has the column on the lane (lane & 31) and the row in the register
// (acc_row), so every store is 32 consecutive floats of one image row.  Lane l feeds point 2s + (l >> 5) of step s: it computes
// its own row weight and column weight in registers, one table interpolation each, from the radial table in LDS.  No weight
// matrix is staged anywhere.
//
// A 32 x 32 tile is reached only by the points within `radius` pixels of it.  Per tile one wave compacts, order preserved
// (ballot + popcount), the indices of the points whose pixel coordinates lie within `radius` of the tile's edges (conservative:
// a superset by half a pixel; a point outside it has an exactly zero weight in every row or every column of the tile, and a
// zero product leaves an fmaf chain unchanged), pads the list to a multiple of eight entries with an index whose weights are
// zero, and runs the chain over the list only, four MFMA steps at a time so that the LDS reads of their operands overlap.  The
// worst case, every point in one pixel, is a list of len entries: the dense product of that tile.
//
// Forward: one workgroup per (frame, 32 image rows), four waves; wave w takes column tiles w, w + 4, ...  LDS: the frame, the
// table (at most 1025 floats), one list of up to len + 7 16-bit indices per wave.
//
// Backward: one workgroup per frame.  The tiles are visited in row-major order, four at a time (one per wave): in log mode the
// wave rebuilds the tile's list and D with the forward's code, then every wave leaves g = dout * scale * inv_norm (log: / (ln 10
// (v + floor))) of its tile in LDS.  Then thread n % 256, the only one that ever touches dx[., ., n], gathers for its point n
// the pixels of these tiles within its reach: per tile (ascending), per row r (ascending) the fmaf chain over the columns c
// (ascending) of g[r][c] b'[n][c] resp. g[r][c] b[n][c], folded into the point's sums with one fmaf by a[n][r] resp. a'[n][r].
// No atomics, no dependence on timing: two runs agree bit for bit.
#include <math.h>

#include "frames.h"
#include "iqvit.h"
#include "prof.h"

namespace {

constexpr int CN_TILE = FR_TILE;
constexpr int CN_TS = CN_TILE + 1;                    // LDS row stride of a g tile
constexpr int CN_MAX_RADIUS = 16, CN_MAX_FRAC = 64;
constexpr int CN_TAB_FLOATS = (CN_MAX_RADIUS * CN_MAX_FRAC + 1 + 3) & ~3;   // the table in LDS, rounded up to 16 bytes
constexpr unsigned CN_PAD = 0xFFFFu;                  // list entry of the padding point (len * 8 <= 64 KB: never an index)
constexpr float CN_LN10 = 2.30258509299404568402f;

constexpr int CN_GROUP = 8;                           // list entries per pass of the chain: four MFMA steps of two points

// 32-bit words of one wave's list: len indices and up to CN_GROUP - 1 padding entries, 16 bits each
__host__ __device__ inline int list_words(int len) { return (len + CN_GROUP) / 2; }

struct CnArgs {
  const float* x;
  const float* table;
  float* out;          // forward
  const float* dout;   // backward
  float* dx;           // backward
  int len;
  iq_constellation_t p;
  int vec4;            // every frame of x starts 16-byte aligned and has a multiple of 4 floats: float4 staging loads
};

// What the weight of a point needs besides its sample: the axis' scale and offset, n_frac and radius * n_frac as floats
struct CnAxis {
  float scale, off, nf, lim;
};

// The weight of pixel centre `centre` (c + 0.5) for the sample s, and sgn(e) * the slope of the table segment it fell into
// (0 where the weight is 0 because the point is out of reach).  Every rounding as include/iqvit.h states it.
struct CnWeight {
  float w, d;
};
__device__ __forceinline__ CnWeight weight2(float s, const CnAxis& ax, float centre, const float* tab) {
  const float e = __fsub_rn(fmaf(s, ax.scale, ax.off), centre);
  const float t = __fmul_rn(fabsf(e), ax.nf);
  const bool ok = t < ax.lim;                         // a NaN or infinite sample fails this
  // no branch: a lane out of reach interpolates at t = 0 and drops the result, so the table reads of several steps overlap
  const float tc = ok ? t : 0.f;
  const int i = (int)tc;                              // tc >= 0: the truncation is floorf
  const float t0 = tab[i], slope = __fsub_rn(tab[i + 1], t0);
  CnWeight r;
  r.w = ok ? fmaf(__fsub_rn(tc, (float)i), slope, t0) : 0.f;
  r.d = ok ? (e > 0.f ? slope : (e < 0.f ? -slope : 0.f)) : 0.f;
  return r;
}
__device__ __forceinline__ float weight(float s, const CnAxis& ax, float centre, const float* tab) {
  return weight2(s, ax, centre, tab).w;
}

// The points that may reach the tile with rows r0 .. r0 + 31 and columns c0 .. c0 + 31, in ascending order, by one wave;
// -> their number, rounded up to a multiple of CN_GROUP with CN_PAD entries.  The caller puts a barrier between this and the
// first read of the list.
__device__ __forceinline__ int build_list(unsigned short* list, const float* fI, const float* fQ, int len, const CnAxis& ax,
                                          const CnAxis& ay, int r0, int c0, int radius, int lane) {
  const float reach = (float)radius;                  // radius - 0.5 to the outermost centre, and half a pixel of margin
  const float ulo = (float)c0 - reach, uhi = (float)(c0 + CN_TILE) + reach;
  const float vlo = (float)r0 - reach, vhi = (float)(r0 + CN_TILE) + reach;
  int cnt = 0;
  for (int base = 0; base < len; base += IQ_WAVE) {
    const int n = base + lane;
    bool in = false;
    if (n < len) {
      const float u = fmaf(fI[n], ax.scale, ax.off), v = fmaf(fQ[n], ay.scale, ay.off);
      in = u > ulo && u < uhi && v > vlo && v < vhi;
    }
    const unsigned long long m = __ballot(in);
    if (in) list[cnt + __popcll(m & ((1ull << lane) - 1ull))] = (unsigned short)n;
    cnt += __popcll(m);
  }
  const int padded = (cnt + CN_GROUP - 1) & ~(CN_GROUP - 1);
  if (cnt + lane < padded) list[cnt + lane] = (unsigned short)CN_PAD;
  return padded;
}

// The chain of one tile over its list: step s takes the points list[2s] and list[2s + 1].  rc / cc: this lane's row and column
// centre (the A operand's row and the B operand's column are both lane & 31).
__device__ __forceinline__ void tile_chain(f32x16& acc, const unsigned short* list, int cnt, const float* fI, const float* fQ,
                                           const CnAxis& ax, const CnAxis& ay, float rc, float cc, const float* tab, int half) {
  for (int s = 0; s < cnt; s += CN_GROUP) {
    float a[CN_GROUP / 2], b[CN_GROUP / 2];
#pragma unroll
    for (int j = 0; j < CN_GROUP / 2; ++j) {                    // the operands of four steps: their LDS reads overlap
      const unsigned n = list[s + 2 * j + half];
      const bool pad = n == CN_PAD;
      const unsigned nc = pad ? 0u : n;
      a[j] = weight(pad ? NAN : fQ[nc], ay, rc, tab);           // a NaN sample has weight 0
      b[j] = weight(pad ? NAN : fI[nc], ax, cc, tab);
    }
#pragma unroll
    for (int j = 0; j < CN_GROUP / 2; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j], b[j], acc, 0, 0, 0);
  }
}

__device__ __forceinline__ CnAxis x_axis(const iq_constellation_t& p) {
  return CnAxis{p.x_scale, p.x_off, (float)p.n_frac, (float)(p.radius * p.n_frac)};
}
__device__ __forceinline__ CnAxis y_axis(const iq_constellation_t& p) {
  return CnAxis{p.y_scale, p.y_off, (float)p.n_frac, (float)(p.radius * p.n_frac)};
}

__device__ __forceinline__ void stage_table(float* tab, const float* table, int n, int tid) {
  for (int i = tid; i < n; i += FR_THREADS) tab[i] = table[i];
}

__global__ __launch_bounds__(FR_THREADS) void constellation_fwd_kernel(CnArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];   // the frame [2][len] | the table | one list per wave
  const int tid = threadIdx.x, lane = tid & (IQ_WAVE - 1), wave = tid >> 6;
  const int col = lane & 31, half = lane >> 5;
  const int len = a.len, H = a.p.height, W = a.p.width, ntc = W / CN_TILE;
  const long fi = blockIdx.x;
  const int r0 = CN_TILE * blockIdx.y;
  const float* fI = lds;
  const float* fQ = lds + len;
  float* tab = lds + frame_floats(len);
  unsigned short* list = reinterpret_cast<unsigned short*>(tab + CN_TAB_FLOATS + wave * list_words(len));
  const CnAxis ax = x_axis(a.p), ay = y_axis(a.p);
  stage_frame(lds, a.x + fi * 2 * len, len, a.vec4, tid);
  stage_table(tab, a.table, a.p.radius * a.p.n_frac + 1, tid);
  __syncthreads();
  float* out_rows = a.out + ((size_t)fi * H + r0) * W;
  const float rc = (float)(r0 + col) + 0.5f;

  for (int tg = 0; tg < ntc; tg += FR_WAVES) {
    const int c0 = CN_TILE * (tg + wave);
    const bool has = c0 < W;                                    // wave-uniform
    int cnt = 0;
    if (has) cnt = build_list(list, fI, fQ, len, ax, ay, r0, c0, a.p.radius, lane);
    __syncthreads();                                            // the list is in LDS
    if (has) {
      f32x16 acc = {};
      tile_chain(acc, list, cnt, fI, fQ, ax, ay, rc, (float)(c0 + col) + 0.5f, tab, half);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float v = __fmul_rn(acc[r], a.p.inv_norm);
        out_rows[(size_t)acc_row(r, half) * W + c0 + col] =
            scale_shift(a.p.mode ? log10f(__fadd_rn(v, a.p.floor)) : v, a.p.scale, a.p.shift);
      }
    }
    __syncthreads();                                            // the list has been read
  }
}

__global__ __launch_bounds__(FR_THREADS) void constellation_bwd_kernel(CnArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];   // the frame | the table | one g tile per wave | one list per wave
  const int tid = threadIdx.x, lane = tid & (IQ_WAVE - 1), wave = tid >> 6;
  const int col = lane & 31, half = lane >> 5;
  const int len = a.len, H = a.p.height, W = a.p.width, ntc = W / CN_TILE, nt = (H / CN_TILE) * ntc;
  const int radius = a.p.radius;
  const long fi = blockIdx.x;
  const float* fI = lds;
  const float* fQ = lds + len;
  float* tab = lds + frame_floats(len);
  float* gt = tab + CN_TAB_FLOATS;
  unsigned short* list = reinterpret_cast<unsigned short*>(gt + FR_WAVES * CN_TILE * CN_TS + wave * list_words(len));
  const CnAxis ax = x_axis(a.p), ay = y_axis(a.p);
  stage_frame(lds, a.x + fi * 2 * len, len, a.vec4, tid);
  stage_table(tab, a.table, radius * a.p.n_frac + 1, tid);
  float* dxi = a.dx + fi * 2 * len;
  float* dxq = dxi + len;
  for (int n = tid; n < len; n += FR_THREADS) dxi[n] = dxq[n] = 0.f;   // thread n % 256 owns point n from here on
  const float* dout = a.dout + (size_t)fi * H * W;
  __syncthreads();

  for (int t0 = 0; t0 < nt; t0 += FR_WAVES) {
    // ---- g of tile t0 + wave: in log mode from D, recomputed with the forward's list and chain
    const int t = t0 + wave;
    const bool has = t < nt;                                    // wave-uniform
    const int r0 = CN_TILE * (t / ntc), c0 = CN_TILE * (t % ntc);
    int cnt = 0;
    if (has && a.p.mode) cnt = build_list(list, fI, fQ, len, ax, ay, r0, c0, radius, lane);
    __syncthreads();                                            // the list is in LDS; the g tiles of the last round are read
    if (has) {
      f32x16 acc = {};
      if (a.p.mode) tile_chain(acc, list, cnt, fI, fQ, ax, ay, (float)(r0 + col) + 0.5f, (float)(c0 + col) + 0.5f, tab, half);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = acc_row(r, half);
        float g = __fmul_rn(__fmul_rn(dout[(size_t)(r0 + row) * W + c0 + col], a.p.scale), a.p.inv_norm);
        if (a.p.mode) g = g / __fmul_rn(CN_LN10, __fadd_rn(__fmul_rn(acc[r], a.p.inv_norm), a.p.floor));
        gt[(wave * CN_TILE + row) * CN_TS + col] = g;
      }
    }
    __syncthreads();                                            // the g tiles of this round are in LDS
    // ---- the gather: every point takes the pixels of these tiles within its reach
    const int nk = nt - t0 < FR_WAVES ? nt - t0 : FR_WAVES;
    for (int n = tid; n < len; n += FR_THREADS) {
      const float si = fI[n], sq = fQ[n];
      const float u = fmaf(si, ax.scale, ax.off), v = fmaf(sq, ay.scale, ay.off);
      if (!(u > -64.f && u < 512.f && v > -64.f && v < 512.f)) continue;   // out of every pixel's reach (or NaN): stays 0
      // pixel p is within reach when v - radius - 0.5 < p < v + radius - 0.5; a quarter pixel of margin on either side
      const float rf = (float)radius;
      const int plo = (int)floorf(v - rf + 0.25f), phi = (int)floorf(v + rf - 0.25f);
      const int qlo = (int)floorf(u - rf + 0.25f), qhi = (int)floorf(u + rf - 0.25f);
      float di = dxi[n], dq = dxq[n];
      for (int k = 0; k < nk; ++k) {
        const int kr0 = CN_TILE * ((t0 + k) / ntc), kc0 = CN_TILE * ((t0 + k) % ntc);
        const int rlo = max(kr0, plo), rhi = min(kr0 + CN_TILE - 1, phi);
        const int clo = max(kc0, qlo), chi = min(kc0 + CN_TILE - 1, qhi);
        if (rlo > rhi || clo > chi) continue;
        const float* g = gt + (k * CN_TILE - kr0) * CN_TS - kc0;
        for (int r = rlo; r <= rhi; ++r) {
          const CnWeight wa = weight2(sq, ay, (float)r + 0.5f, tab);
          if (wa.w == 0.f && wa.d == 0.f) continue;
          float s1 = 0.f, s2 = 0.f;
          for (int c = clo; c <= chi; ++c) {
            const CnWeight wb = weight2(si, ax, (float)c + 0.5f, tab);
            const float gv = g[r * CN_TS + c];
            s1 = fmaf(gv, wb.d, s1);
            s2 = fmaf(gv, wb.w, s2);
          }
          di = fmaf(wa.w, s1, di);
          dq = fmaf(wa.d, s2, dq);
        }
      }
      dxi[n] = di;
      dxq[n] = dq;
    }
  }
  const float kx = __fmul_rn(a.p.x_scale, ax.nf), ky = __fmul_rn(a.p.y_scale, ay.nf);
  for (int n = tid; n < len; n += FR_THREADS) {
    dxi[n] = __fmul_rn(kx, dxi[n]);
    dxq[n] = __fmul_rn(ky, dxq[n]);
  }
}

bool size_ok(int n) { return n >= FR_MIN_FFT && n <= FR_MAX_FFT && n % FR_TILE == 0; }

// -> IQ_OK or the refusal; nothing is launched and no pointer dereferenced (other than par) before this returns IQ_OK
int check(const void* x, const void* table, const void* io_a, const void* io_b, int len, const iq_constellation_t* p) {
  if (!x || !table || !io_a || !io_b || !p) return IQ_ERR_ARG;
  if (len <= 0 || (p->mode & ~1)) return IQ_ERR_ARG;
  if (!is_finite(p->x_scale) || !is_finite(p->x_off) || !is_finite(p->y_scale) || !is_finite(p->y_off)) return IQ_ERR_ARG;
  if (!is_finite(p->inv_norm) || !is_finite(p->floor) || !is_finite(p->scale) || !is_finite(p->shift)) return IQ_ERR_ARG;
  if (p->mode == 1 && !(p->floor > 0.f)) return IQ_ERR_ARG;
  if (((uintptr_t)x & 3) || ((uintptr_t)table & 3) || ((uintptr_t)io_a & 3) || ((uintptr_t)io_b & 3)) return IQ_ERR_ARG;
  if (!size_ok(p->height) || !size_ok(p->width)) return IQ_ERR_UNSUPPORTED;
  if (p->radius < 1 || p->radius > CN_MAX_RADIUS || p->n_frac < 1 || p->n_frac > CN_MAX_FRAC) return IQ_ERR_UNSUPPORTED;
  if (!frame_fits(len)) return IQ_ERR_UNSUPPORTED;
  return IQ_OK;
}

CnArgs pack(const float* x, const float* table, int len, const iq_constellation_t* p) {
  CnArgs a;
  a.x = x; a.table = table; a.out = nullptr; a.dout = nullptr; a.dx = nullptr; a.len = len; a.p = *p;
  a.vec4 = frame_vec4(x, len);
  return a;
}

}  // namespace

extern "C" int iq_frames_constellation(const float* x, const float* table, float* out, int n_frames, int len,
                                       const iq_constellation_t* par, iq_stream_t stream) {
  const int rc = check(x, table, out, out, len, par);
  if (rc != IQ_OK) return rc;
  if (n_frames <= 0) return IQ_OK;
  hipStream_t st = (hipStream_t)stream;
  IQ_PROF(IQ_FAM_MISC, st);
  CnArgs a = pack(x, table, len, par);
  a.out = out;
  const size_t lds = ((size_t)frame_floats(len) + CN_TAB_FLOATS + FR_WAVES * list_words(len)) * sizeof(float);
  const double px = (double)n_frames * par->height * par->width;
  IQ_PROF_K((double)n_frames * len * 8 + px * 4, 2.0 * px * len, "constellation_fwd_kernel");
  launch_frames(constellation_fwd_kernel, dim3(n_frames, par->height / CN_TILE), lds, st, a);
  return iq_launch_status();
}

extern "C" int iq_frames_constellation_bwd(const float* x, const float* table, const float* dout, float* dx, int n_frames,
                                           int len, const iq_constellation_t* par, iq_stream_t stream) {
  const int rc = check(x, table, dout, dx, len, par);
  if (rc != IQ_OK) return rc;
  if (n_frames <= 0) return IQ_OK;
  hipStream_t st = (hipStream_t)stream;
  IQ_PROF(IQ_FAM_MISC, st);
  CnArgs a = pack(x, table, len, par);
  a.dout = dout; a.dx = dx;
  const size_t lds =
      ((size_t)frame_floats(len) + CN_TAB_FLOATS + FR_WAVES * CN_TILE * CN_TS + FR_WAVES * list_words(len)) * sizeof(float);
  const double px = (double)n_frames * par->height * par->width;
  IQ_PROF_K((double)n_frames * len * 16 + px * 4, 6.0 * px * len, "constellation_bwd_kernel");
  launch_frames(constellation_bwd_kernel, n_frames, lds, st, a);
  return iq_launch_status();
}
