// One-wave probes that keep the hardware assumptions of the attention
// kernels verified on silicon: the fragment layouts of the two bf16 MFMA
// shapes and the semantics of the LDS transpose read.  Test-only: nothing on
// the training path launches them.
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

#include "mfma_frag.h"

namespace {

// Verifies the assumed A/B fragment layouts: C[16][16] = A[16][32]·B[32][16]
// with A,B read from global memory exactly the way the v1 attention kernels
// read their fragments.
__global__ void mfma_probe_kernel(const bf16* __restrict__ A,
                                  const bf16* __restrict__ Bt,
                                  float* __restrict__ C) {
    const int lane = threadIdx.x;
    const int lgrp = lane >> 4, lcol = lane & 15;
    // A[m][k]: m = lcol, k = 8*lgrp + i  (row-major A: 16x32)
    frag_ab a = *reinterpret_cast<const frag_ab*>(A + lcol * 32 + 8 * lgrp);
    // B[k][n] with Bt stored as [n][k] (row-major 16x32): n = lcol, k = 8*lgrp+i
    frag_ab b = *reinterpret_cast<const frag_ab*>(Bt + lcol * 32 + 8 * lgrp);
    frag_cd c = MFMA_16x16x32(a, b, frag_cd{0.f, 0.f, 0.f, 0.f});
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        C[(4 * lgrp + r) * 16 + lcol] = c[r];
    }
}

// layout probe for the 32x32x16 fragment maps (see attn_fwd_v2_kernel)
__global__ void mfma_probe32_kernel(const bf16* __restrict__ A,
                                    const bf16* __restrict__ Bt,
                                    float* __restrict__ C) {
    const int lane = threadIdx.x;
    const int l31 = lane & 31, hi = lane >> 5;
    // A[i][k]: i = l31, k = 8*hi + e (row-major A: 32x16)
    frag_ab a = *reinterpret_cast<const frag_ab*>(A + l31 * 16 + 8 * hi);
    // B[k][j] with Bt stored [j][k] (row-major 32x16): j = l31, k = 8*hi + e
    frag_ab b = *reinterpret_cast<const frag_ab*>(Bt + l31 * 16 + 8 * hi);
    f32x16 c;
#pragma unroll
    for (int r = 0; r < 16; ++r) c[r] = 0.f;
    c = MFMA_32x32x16(a, b, c);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        C[((r & 3) + 8 * (r >> 2) + 4 * hi) * 32 + l31] = c[r];
    }
}

// semantics probe for ds_read_b64_tr_b16: stage a [4][16] bf16 tile into
// LDS, read it with the transpose instruction the way the v2 PV loop does,
// and write out what each lane received (expected: lane l&15 gets column
// l&15, elements j=0..3 = rows).
__global__ void tr16_probe_kernel(const bf16* __restrict__ in,
                                  float* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) bf16 lds[64];
    const int lane = threadIdx.x;
    if (lane < 8) {
        *reinterpret_cast<frag_ab*>(&lds[lane * 8]) =
            *reinterpret_cast<const frag_ab*>(in + lane * 8);
    }
    __syncthreads();
    if (lane < 16) {
        bf16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
            (lds_bf16x4_p)&lds[lane * 4]);
#pragma unroll
        for (int j = 0; j < 4; ++j) out[lane * 4 + j] = (float)v[j];
    }
}

}  // namespace

torch::Tensor mfma_probe(torch::Tensor A, torch::Tensor Bt) {
    TORCH_CHECK(A.is_cuda() && A.scalar_type() == torch::kBFloat16);
    TORCH_CHECK(A.sizes() == torch::IntArrayRef({16, 32}) &&
                Bt.sizes() == torch::IntArrayRef({16, 32}));
    auto C = torch::empty({16, 16}, A.options().dtype(torch::kFloat));
    auto stream = at::cuda::getCurrentCUDAStream();
    hipLaunchKernelGGL(mfma_probe_kernel, dim3(1), dim3(64), 0, stream,
        reinterpret_cast<const bf16*>(A.contiguous().data_ptr()),
        reinterpret_cast<const bf16*>(Bt.contiguous().data_ptr()),
        C.data_ptr<float>());
    HIP_CHECK_LAUNCH();
    return C;
}

torch::Tensor mfma_probe32(torch::Tensor A, torch::Tensor Bt) {
    TORCH_CHECK(A.is_cuda() && A.scalar_type() == torch::kBFloat16);
    TORCH_CHECK(A.sizes() == torch::IntArrayRef({32, 16}) &&
                Bt.sizes() == torch::IntArrayRef({32, 16}));
    auto C = torch::empty({32, 32}, A.options().dtype(torch::kFloat));
    auto stream = at::cuda::getCurrentCUDAStream();
    hipLaunchKernelGGL(mfma_probe32_kernel, dim3(1), dim3(64), 0, stream,
        reinterpret_cast<const bf16*>(A.contiguous().data_ptr()),
        reinterpret_cast<const bf16*>(Bt.contiguous().data_ptr()),
        C.data_ptr<float>());
    HIP_CHECK_LAUNCH();
    return C;
}

torch::Tensor tr16_probe(torch::Tensor tile) {
    TORCH_CHECK(tile.is_cuda() && tile.scalar_type() == torch::kBFloat16 &&
                tile.numel() == 64);
    auto out = torch::empty({16, 4}, tile.options().dtype(torch::kFloat));
    auto stream = at::cuda::getCurrentCUDAStream();
    hipLaunchKernelGGL(tr16_probe_kernel, dim3(1), dim3(64), 0, stream,
        reinterpret_cast<const bf16*>(tile.contiguous().data_ptr()),
        out.data_ptr<float>());
    HIP_CHECK_LAUNCH();
    return out;
}
