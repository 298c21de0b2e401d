// The fixed-order slab reduce of the weight-gradient family, as device functions two kernels share:
// wgrad_reduce_kernel (gemm_wgrad.hip), one workgroup per virtual block, and the reduce role of gemm_lnbwd_kernel
// (gemm_lnbwd.hip), where the workgroups that the row tiles leave free walk the virtual blocks of a job.
//
//   out[i] (+)= sum_s slab[s][i]   for up to 2*RED_MAXP + RED_MAXX segments (weights and biases of a group + extra)
//
// A virtual block = 256 threads on one segment.  "wide" = 64 float4 columns x 4 row slices (few slab rows, many columns:
// coalesced 1 KiB rows, 4x the loads in flight of a one-thread-per-column loop), "tall" = 16 columns x 16 slices (hundreds
// of LayerNorm partial rows, 192 columns): keeps every thread's serial chain short either way.  The arithmetic is the
// same wherever a block runs, so the bits are: per column, slice sl sums rows sl, sl + nsl, ... in increasing order from
// 0.f; the slices meet in LDS and are added in order 0, 1, 2, ...; out = accumulate ? out + t : t.
#pragma once
#include "common.h"

constexpr int RED_THREADS = 256;
constexpr int RED_MAXP = 4;   // problems of a group (PW_MAXP, gemm_wgrad.hip)
constexpr int RED_MAXX = 4;   // extra (LayerNorm partial) segments
static_assert(IQ_REDUCE_JOB_SEGS == 2 * RED_MAXP + RED_MAXX, "iq_reduce_job_t holds a group's segments");
typedef iq_reduce_job_seg_t RedSeg;     // { partials (slab rows), out, n, stride, rows, blk0, tall }
typedef iq_reduce_job_t RedGroup;       // { seg[], nseg, nblk, accumulate }

inline int red_blocks(long n, int tall) { return (int)((n + (tall ? 63 : 255)) / (tall ? 64 : 256)); }

// a thread's share of virtual block vb: float4 column `i` of slice `sl`
struct RedLane {
  const float* slab; float* out;
  long n, stride, i;
  int rows, ncol, nsl, col, sl;
};
__device__ __forceinline__ RedLane red_lane(const RedGroup& g, int vb) {
  RedSeg sg = g.seg[0];
#pragma unroll
  for (int i = 1; i < 2 * RED_MAXP + RED_MAXX; ++i)
    if (i < g.nseg && vb >= g.seg[i].blk0) sg = g.seg[i];
  RedLane l;
  l.slab = sg.partials; l.out = sg.out; l.n = sg.n; l.stride = sg.stride; l.rows = sg.rows;
  const long blk = (long)vb - sg.blk0;
  l.ncol = sg.tall ? 16 : 64; l.nsl = RED_THREADS / l.ncol;
  l.col = threadIdx.x % l.ncol; l.sl = threadIdx.x / l.ncol;
  l.i = (blk * l.ncol + l.col) * 4;
  return l;
}
// the scalar tail of a segment whose n is no multiple of 4 (the last float4 column)
__device__ __forceinline__ void red_tail_sum(const RedLane& l, f32x4& s) {
  for (int sp = l.sl; sp < l.rows; sp += l.nsl)
    for (int e = 0; e < 4 && l.i + e < l.n; ++e) s[e] += l.slab[(long)sp * l.stride + l.i + e];
}
// slices 0, 1, 2, ... of this thread's column from `part` (after the barrier), then the output
__device__ __forceinline__ void red_combine(const RedLane& l, const f32x4* part, int accumulate) {
  if (l.sl == 0 && l.i < l.n) {
    f32x4 t = part[l.col];
    for (int k = 1; k < l.nsl; ++k) t += part[k * l.ncol + l.col];
    if (l.i + 4 <= l.n) {
      f32x4* o = reinterpret_cast<f32x4*>(l.out + l.i);
      *o = accumulate ? *o + t : t;
    } else {
      for (int e = 0; e < 4 && l.i + e < l.n; ++e) l.out[l.i + e] = accumulate ? l.out[l.i + e] + t[e] : t[e];
    }
  }
}

// One virtual block by one workgroup.  part: RED_THREADS float4 of LDS.
__device__ __forceinline__ void red_block(const RedGroup& g, int vb, f32x4* part) {
  const RedLane l = red_lane(g, vb);
  const float* __restrict__ slab = l.slab;
  f32x4 s = {0.f, 0.f, 0.f, 0.f};
  if (l.i + 4 <= l.n) {
#pragma unroll 8
    for (int sp = l.sl; sp < l.rows; sp += l.nsl) s += *reinterpret_cast<const f32x4*>(slab + (long)sp * l.stride + l.i);
  } else if (l.i < l.n) {
    red_tail_sum(l, s);
  }
  part[l.sl * l.ncol + l.col] = s;
  __syncthreads();
  red_combine(l, part, g.accumulate);
}

// Virtual blocks first, first + step, ... < g.nblk by one workgroup, one after the other.  A lone workgroup has nobody
// to hide its load latency behind, so a thread requests ROWS rows of its column before the first sum (ROWS float4 in
// flight per thread); the sums run in the order of red_block.  part: RED_THREADS float4 of LDS.
template <int ROWS>
__device__ __forceinline__ void red_walk(const RedGroup& g, int first, int step, f32x4* part) {
  for (int vb = first; vb < g.nblk; vb += step) {
    const RedLane l = red_lane(g, vb);
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    if (l.i + 4 <= l.n) {
      for (int sp0 = l.sl; sp0 < l.rows; sp0 += ROWS * l.nsl) {
        f32x4 v[ROWS];
#pragma unroll
        for (int u = 0; u < ROWS; ++u) {
          const int sp = sp0 + u * l.nsl;
          v[u] = f32x4{0.f, 0.f, 0.f, 0.f};
          if (sp < l.rows) v[u] = *reinterpret_cast<const f32x4*>(l.slab + (long)sp * l.stride + l.i);
        }
#pragma unroll
        for (int u = 0; u < ROWS; ++u)
          if (sp0 + u * l.nsl < l.rows) s += v[u];
      }
    } else if (l.i < l.n) {
      red_tail_sum(l, s);
    }
    part[l.sl * l.ncol + l.col] = s;
    __syncthreads();
    red_combine(l, part, g.accumulate);
    __syncthreads();                                                     // the next block overwrites `part`
  }
}
