// The pieces the attention kernels share (attention.hip: the (frame, head) kernels, attn_bwd_once_kernel and the per-frame
// kernels; attn_maps.hip: the read-back kernels), each defined once.  Everything here takes plain values and pointers and
// knows nothing of the kernel that calls it.  Every kernel compiles to the machine code it had with its own copy
// (profiles/attn_common_refactor.txt, which also lists what was tried and stays written out in the kernels).
//   device  LOG2E / LN2 / NEG_BIG, fast_exp2, AttCfg, the LDS layouts (Rows / HeadRows, RowsRt, Swizzle64), row_frag, tr_frag,
//           pack_b, rebuild_p_ds, group4_max / group4_sum
//   host    padded32, launch_lds, dispatch_dh
#pragma once
#include <math.h>

#include <type_traits>

#include "common.h"

constexpr float LOG2E = 1.4426950408889634f;
constexpr float LN2 = 0.6931471805599453f;
constexpr float NEG_BIG = -1.0e30f;

// exp2 for softmax arguments (<= 0 after the max / LSE subtraction): the bare v_exp_f32.  exp2f() wraps it in a
// denormal-range fix-up (compare, select, add, select, ldexp: five extra VALU instructions per value) that only matters
// for results below 2^-126, which are zero for every purpose here -- and the attention kernels are VALU-bound.
__device__ __forceinline__ float fast_exp2(float x) { return __builtin_amdgcn_exp2f(x); }

// LDS images of a head slice are [rows][dh + 16] bf16 (32 B pad: conflict-free transposed reads, 2-way on row reads).
template <int DH> struct AttCfg {
  static constexpr int LD = (DH == 16) ? 16 : DH + 16;  // LDS row stride (elements)
  static constexpr int KS = (DH + 31) / 32;              // 32-deep contraction steps over d
  static constexpr int DT = DH / 16;                     // 16-wide d tiles
  static constexpr int CPR = DH / 8;                     // 16 B chunks per row
};

// ---- LDS layouts: where element (row, col + dcol) of an image lies.  A stride that is a constant reaches the address
// arithmetic as a constant (Rows<LD>); passed as an `int` it cost the dh = 16 kernels up to 203 lines of assembly each.
// dcol is the lane's place inside a 16-column tile at col: one address, but the sum is formed in the order each kernel's
// own copy formed it (linear rows add it last, the swizzle takes the whole column), which the instruction schedule follows.
// step(): 16 rows further down, for every layout a plain distance.
template <int LD> struct Rows {          // compile-time row stride: the (frame, head) kernels and the read-back kernels
  template <class T>
  __device__ __forceinline__ T* operator()(T* img, int row, int col, int dcol = 0) const {
    return img + row * LD + col + dcol;
  }
  __device__ __forceinline__ int step() const { return 16 * LD; }
};
template <int DH> using HeadRows = Rows<AttCfg<DH>::LD>;   // a head slice's image [rows][AttCfg<DH>::LD]
struct RowsRt {                          // run-time row stride: the per-frame images [spad][3 D + 16] and [spad][D + 16]
  int ld;
  template <class T>
  __device__ __forceinline__ T* operator()(T* img, int row, int col, int dcol = 0) const {
    return img + row * ld + col + dcol;
  }
  __device__ __forceinline__ int step() const { return 16 * ld; }
};
// attn_bwd_once_kernel's unpadded 128-byte rows, XOR-swizzled: the 32-byte column pair p of row r lives at pair
// p ^ ((r >> 1) & 3).  A 32-lane half of a transposed read covers 8 consecutive rows x 32 B, of a row read 16 lanes cover
// 16 rows x 16 B: either way every 16-byte slot of the 256-byte bank row exactly once (conflict-free; the padded 160-byte rows
// were 2-way on row reads).  Row + 16 has the same swizzle.
constexpr int ONCE_LD = 64;              // Q / dO / K image row stride (elements): no pad, swizzled
struct Swizzle64 {
  template <class T>
  __device__ __forceinline__ T* operator()(T* img, int row, int col, int dcol = 0) const {
    return img + (row * ONCE_LD + ((col + dcol) ^ (((row >> 1) & 3) << 4)));
  }
  __device__ __forceinline__ int step() const { return 16 * ONCE_LD; }
};

typedef __attribute__((address_space(3))) s16x4 lds_s16x4;

// row-major fragment: 8 consecutive d of row `row`, contraction step s (d0 = 32 s + 8 g); dh = 16 zero-pads the contraction
template <int DH, class Off>
__device__ __forceinline__ bf16x8 row_frag(const bf16* tile, Off off, int row, int s, int lane) {
  const int d0 = s * 32 + 8 * (lane >> 4);
  bf16x8 v = {};
  if (DH >= 32 || d0 < DH) v = *reinterpret_cast<const bf16x8*>(off(tile, row, d0));
  return v;
}
// transposed fragment (ds_read_b64_tr_b16 twice): lane group g gets rows {4g..4g+3} U {16+4g..16+4g+3} of the 32 rows from r0,
// columns c0 .. c0+15: what two stacked 16x16 accumulator tiles hold.  (K-slot order inside an MFMA is free as long as A and
// B agree, which is what lets an accumulator tile be the next product's operand as it stands.)
template <class Off>
__device__ __forceinline__ bf16x8 tr_frag(const bf16* tile, Off off, int r0, int c0, int lane) {
  const int i16 = lane & 15, g = lane >> 4;
  const bf16* a = off(tile, r0 + 4 * g + (i16 >> 2), c0, 4 * (i16 & 3));
  s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(a));
  s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(a + off.step()));
  s16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(bf16x8, v);
}

__device__ __forceinline__ bf16x8 pack_b(const f32x4& lo, const f32x4& hi) {
  bf16x8 v;
#pragma unroll
  for (int r = 0; r < 4; ++r) { v[r] = (bf16)lo[r]; v[4 + r] = (bf16)hi[r]; }
  return v;
}

// Backward, key on the lane: P and dS of one 16 x 16 tile (4 queries x this lane's key) rebuilt from its scores sa, dP, the
// queries' lse (log2 domain) and delta.  Padded QUERY rows need no mask: Q = dO = 0 and lse = delta = 0 there, so P = 1 and
// dS = 0 multiply zeros.  Padded KEYS do (key_live false; only a unit_partial wave can hold them): P = exp2(-lse) is unbounded
// when a row's scores are all very negative, and inf * 0 would poison dQ.  Arguments by value: by reference
// attn_bwd_once_kernel's schedule moved.
__device__ __forceinline__ void rebuild_p_ds(f32x4 sa, f32x4 dp, f32x4 lq4, f32x4 dl4, float scale_log2,
                                             float scale, bool unit_partial, bool key_live, f32x4& p, f32x4& ds) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    float pv = fast_exp2(sa[r] * scale_log2 - lq4[r]);
    if (unit_partial) pv = key_live ? pv : 0.f;
    p[r] = pv;
    ds[r] = pv * (dp[r] - dl4[r]) * scale;
  }
}

__device__ __forceinline__ float group4_max(float v) {  // across lane groups (lanes l, l^16, l^32, l^48)
  v = fmaxf(v, __shfl_xor(v, 16, 64));
  return fmaxf(v, __shfl_xor(v, 32, 64));
}
__device__ __forceinline__ float group4_sum(float v) {
  v += __shfl_xor(v, 16, 64);
  return v + __shfl_xor(v, 32, 64);
}

// ---- host
// sequence length in whole 32-row tiles
constexpr int padded32(int S) { return (S + 31) / 32 * 32; }

// Launch with `lds` bytes of dynamic LDS: above the default 48 KB cap the kernel's cap is raised first (on every such launch).
template <class... P, class... A>
inline int launch_lds(void (*kernel)(P...), unsigned grid, int threads, size_t lds, hipStream_t st, const A&... args) {
  if (lds > 48 * 1024) (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  kernel<<<grid, threads, lds, st>>>(static_cast<P>(args)...);
  return iq_launch_status();
}

// f(std::integral_constant<int, dh>) for the head widths the kernels are built for
template <class F> inline int dispatch_dh(int dh, F&& f) {
  switch (dh) {
    case 16: return f(std::integral_constant<int, 16>{});
    case 32: return f(std::integral_constant<int, 32>{});
    case 64: return f(std::integral_constant<int, 64>{});
    default: return IQ_ERR_UNSUPPORTED;
  }
}
