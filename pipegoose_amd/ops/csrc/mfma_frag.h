// bf16 MFMA fragment types and intrinsic wrappers shared by the attention
// kernels (attention.hip) and the layout probes that keep their fragment
// maps verified on silicon (probes.hip).
#pragma once

#include "common.h"

using bf16 = __hip_bfloat16;
using frag_ab = __attribute__((ext_vector_type(8))) __bf16;   // 8 bf16 = 4 VGPR
using frag_cd = __attribute__((ext_vector_type(4))) float;    // 4 fp32
using f32x16 = __attribute__((ext_vector_type(16))) float;
using f32x4 = __attribute__((ext_vector_type(4))) float;
using bf16x4 = __attribute__((ext_vector_type(4))) __bf16;
using lds_bf16x4_p = __attribute__((address_space(3))) bf16x4*;

// v_mfma_f32_16x16x32_bf16
//   A-fragment (M=16 side): row = lane&15, k = 8*(lane>>4) + i
//   B-fragment (N=16 side): col = lane&15, k = 8*(lane>>4) + i
//   C/D:                    col = lane&15, row = 4*(lane>>4) + reg
// (verified by mfma_probe)
__device__ __forceinline__ frag_cd MFMA_16x16x32(frag_ab a, frag_ab b, frag_cd c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

// v_mfma_f32_32x32x16_bf16
//   A/B fragments: i/j = lane&31, k = 8*(lane>>5) + elem
//   C/D:           col = lane&31, row = (r&3) + 8*(r>>2) + 4*(lane>>5),
//                  r in [0,16)
// (verified by mfma_probe32)
__device__ __forceinline__ f32x16 MFMA_32x32x16(frag_ab a, frag_ab b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}
