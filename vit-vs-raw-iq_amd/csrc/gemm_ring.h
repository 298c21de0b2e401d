// What gemm_nt_async_kernel (gemm_nt.hip), gemm_ln_kernel (gemm_ln.hip) and gemm_lnbwd_kernel (gemm_lnbwd.hip) share of
// their main loop: operands stream HBM -> LDS with global_load_lds_dwordx4 (no VGPR staging) through a 3-slot ring of
// 32-deep K stages, two stages in flight behind the one being multiplied, counted s_waitcnt vmcnt + raw s_barrier.
// 256 threads = 4 waves as 2 (rows) x 2 (columns); a wave multiplies BMT/2 rows x BN/2 columns of the BMT x BN tile.
// Stage = [BMT + BN rows][64 B]; 16 B chunk c of row r sits at chunk c ^ f(r>>2), f = {0,2,3,1} (chosen so that the
// 16-lane groups of ds_read_b128, which mix lanes of chunk c and c+1, hit 16 distinct slots): the DMA writes LDS
// lane-linearly, so the swizzle is applied to the per-lane SOURCE address and again on the ds_read_b128 fragment
// reads, which are then bank-conflict free.
// Here: the ring's geometry, the swizzle, the stage-head wait and the de-phasing offset.  The address setup, issue and
// multiply bodies are still written out in each kernel: moved into helpers here they compiled to different (reordered)
// machine code, and these kernels' counted waits are checked against the ISA (scripts/dbg/check_epi_counts.py).
#pragma once
#include <utility>

#include "common.h"

template <int BMT, int BN>
struct RingShape {
  static constexpr int BK2 = 32, NS = 3;                           // stage depth (K), slots
  static constexpr int WN = BN / 2, NT = WN / 16, MT = BMT / 32;   // wave tile = BMT/2 rows x BN/2 cols, in 16 x 16 MFMA tiles
  static constexpr int STAGE_BYTES = (BMT + BN) * BK2 * 2;
  static constexpr int BYTES = NS * STAGE_BYTES;
  static constexpr int A_LD = BMT * BK2 * 2 / (4 * 1024);          // 1 KiB DMA pieces per wave per stage: A 2 | 1
  static constexpr int B_LD = BN * BK2 * 2 / (4 * 1024);           //                                      B 3 | 2 | 1
  static constexpr int PER_STAGE = A_LD + B_LD;
  static constexpr int NRS = BN / BK2;                             // residual stages of a whole-row tile (RESK, gemm_nt.hip)
  static_assert(NT % 2 == 0 && A_LD >= 1 && B_LD >= 1, "tile shape");
};

__device__ __forceinline__ int ring_swz64(int row) { return (0x78 >> (((row >> 2) & 3) * 2)) & 3; }

// Co-resident workgroups otherwise run their phases in lockstep (all waiting on HBM, then all on the MFMA pipe, then
// all storing): each kernel de-phases them once at launch by this workgroup's phase (0..3) x its stagger x s_sleep(8)
// (~512 cycles each); the offset persists as slots are refilled.
__device__ __forceinline__ int ring_phase() { return (int)(((unsigned)blockIdx.x * 2654435761u) >> 30); }

// Head of a stage: all but the youngest N entries of this wave's in-order vector-memory queue have landed, then
// everyone's have (the barrier also says that the stage multiplied before it is no longer read).  Where N depends on a
// run-time condition, only wait_vmcnt goes under the branches and ONE ring_barrier follows them.
template <int N>
__device__ __forceinline__ void wait_vmcnt() { asm volatile("s_waitcnt vmcnt(%0)" :: "n"(N) : "memory"); }
__device__ __forceinline__ void ring_barrier() {
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}
template <int N>
__device__ __forceinline__ void wait_barrier() {
  wait_vmcnt<N>();
  ring_barrier();
}

// f(integral_constant<int, 0>) ... f(integral_constant<int, N - 1>): stages whose accumulator indices must be static
template <int... T, class F>
__device__ __forceinline__ void static_for(std::integer_sequence<int, T...>, F&& f) {
  (f(std::integral_constant<int, T>{}), ...);
}
template <int N, class F>
__device__ __forceinline__ void static_for(F&& f) { static_for(std::make_integer_sequence<int, N>{}, f); }
