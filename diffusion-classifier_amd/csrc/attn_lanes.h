// attn_lanes.h — reductions over the four lanes that share a query column in the transposed-score attention kernels
// (attention.hip: self-attention's flash and wave kernels; attn_strip.h: the body of cross-, bias and causal attention).
#pragma once
#include "common.h"

// Reductions over the four lanes that share a query column in the transposed-score form (lanes lr, lr + 16, lr + 32, lr + 48) on the
// VALU: v_permlane16_swap_b32 exchanges the odd 16-lane rows of one operand with the even rows of the other, v_permlane32_swap_b32 the
// upper half of one with the lower half of the other — with both operands the same register the two results are "rows 0 0 2 2" /
// "rows 1 1 3 3" and "lower lower" / "upper upper", so an op over each pair is the xor-16 / xor-32 butterfly.  The ds_bpermute shuffles
// these replace were four LDS round trips per query tile and key block in front of the exponentials.
// (as instructions, not through __builtin_amdgcn_permlane{16,32}_swap: hipcc 7.2 folds the builtin's two results into one once they meet in
//  an add or a max — it emitted v_add_f32 v, a0, a0 for a0 + a1, with the same or with different operands — which the hardware does not
//  do: tools/dev/permlane_probe.hip prints what the instruction returns.  The two wait states in front cover a VALU write of the
//  operands, as the compiler places them in front of its own.)
template <bool WIDE> static __device__ __forceinline__ void lane_swap(float x, float& lo, float& hi) {
  unsigned u = __builtin_bit_cast(unsigned, x), v = u;
  if constexpr (WIDE) asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(u), "+v"(v));
  else asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(u), "+v"(v));
  lo = __builtin_bit_cast(float, u); hi = __builtin_bit_cast(float, v);
}
static __device__ __forceinline__ float col4_max(float x) {
  float a, b;
  lane_swap<false>(x, a, b);
  lane_swap<true>(fmaxf(a, b), a, b);
  return fmaxf(a, b);
}
static __device__ __forceinline__ float col4_sum(float x) {
  float a, b;
  lane_swap<false>(x, a, b);
  lane_swap<true>(a + b, a, b);
  return a + b;
}
