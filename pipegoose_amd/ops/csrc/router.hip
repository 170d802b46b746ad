// Fused Switch-Transformer router for gfx950 (north-star kernel list).
//
// One pass over the [N, E] gate logits produces everything the MoE layer
// needs: per-token top-k expert ids + routing probs, the per-expert
// probability column sums (Switch aux-loss term P_i), per-expert top-1
// counts (f_i), and per-token logsumexp (ST-MoE z-loss) — instead of the
// softmax → topk → scatter → mean → logsumexp chain of separate kernels.
// E <= 64 (one expert per lane); the inference/dispatch path of the router
// (the training path keeps torch autograd ops for the loss gradients).
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

#include "common.h"

namespace {

constexpr int RT_BLOCK = 256;
constexpr int RT_WAVES = RT_BLOCK / WAVE_SIZE;

// A wave walks rows_per_wave consecutive token rows and keeps its column sums
// and top-1 counts in registers; the block adds its waves in a fixed order and
// issues ONE atomic per expert.  One fp32 atomic per row and expert summed N
// terms at full magnitude in arrival order (colsum 9e-4 off at N=4097, sum
// 512: 25x the error of a torch sum); now N / (RT_WAVES * rows_per_wave) do.
template <typename T, int K>
__global__ void router_topk_kernel(
    const T* __restrict__ logits,
    int* __restrict__ topk_idx, float* __restrict__ topk_val,
    float* __restrict__ prob_colsum, int* __restrict__ top1_count,
    float* __restrict__ lse, int64_t N, int E, int rows_per_wave) {
    __shared__ float s_p[RT_WAVES][WAVE_SIZE];
    __shared__ int s_c[RT_WAVES][WAVE_SIZE];
    // lane e holds expert e
    const int wave = threadIdx.x / WAVE_SIZE;
    const int lane = threadIdx.x % WAVE_SIZE;
    const int64_t row0 = ((int64_t)blockIdx.x * RT_WAVES + wave) * rows_per_wave;

    float psum = 0.f;
    int cnt = 0;
    for (int rr = 0; rr < rows_per_wave; ++rr) {
        const int64_t row = row0 + rr;
        if (row >= N) break;  // wave-uniform

        float x = (lane < E) ? to_float(logits[row * E + lane]) : -1e30f;
        float mx = wave_reduce_max(x);
        mx = __shfl(mx, 0, WAVE_SIZE);
        float ex = (lane < E) ? __expf(x - mx) : 0.f;
        float denom = wave_reduce_sum(ex);
        denom = __shfl(denom, 0, WAVE_SIZE);
        const float p = ex / denom;

        psum += p;  // lanes >= E add 0
        if (lane == 0) lse[row] = mx + __logf(denom);

        // top-k by repeated masked max (K is 1 or 2)
        float pv = p;
#pragma unroll
        for (int kk = 0; kk < K; ++kk) {
            float best = wave_reduce_max(pv);
            best = __shfl(best, 0, WAVE_SIZE);
            // lowest lane holding the max wins
            const bool is_best = (pv == best) && (lane < E);
            unsigned long long mask = __ballot(is_best);
            const int win = __ffsll((unsigned long long)mask) - 1;
            if (lane == win) {
                topk_idx[row * K + kk] = lane;
                topk_val[row * K + kk] = p;
                if (kk == 0) ++cnt;
                pv = -1.f;  // exclude from the next round
            }
        }
    }

    s_p[wave][lane] = psum;
    s_c[wave][lane] = cnt;
    __syncthreads();
    if (wave == 0 && lane < E) {
        float tp = s_p[0][lane];
        int tc = s_c[0][lane];
#pragma unroll
        for (int w = 1; w < RT_WAVES; ++w) {
            tp += s_p[w][lane];
            tc += s_c[w][lane];
        }
        atomicAdd(&prob_colsum[lane], tp);
        if (tc != 0) atomicAdd(&top1_count[lane], tc);
    }
}

}  // namespace

std::vector<torch::Tensor> router_topk(torch::Tensor logits, int64_t k) {
    TORCH_CHECK(logits.is_cuda() && logits.is_contiguous() && logits.dim() == 2);
    TORCH_CHECK(k == 1 || k == 2, "router_topk: k must be 1 or 2");
    const int64_t N = logits.size(0);
    const int E = logits.size(1);
    TORCH_CHECK(E <= 64, "router_topk: at most 64 experts (one per lane)");

    auto opts_f = logits.options().dtype(torch::kFloat);
    auto opts_i = logits.options().dtype(torch::kInt);
    auto topk_idx = torch::empty({N, k}, opts_i);
    auto topk_val = torch::empty({N, k}, opts_f);
    auto colsum = torch::zeros({E}, opts_f);
    auto count = torch::zeros({E}, opts_i);
    auto lse = torch::empty({N}, opts_f);

    // 16 rows per wave, more once that would pass 256 blocks: at most 256
    // atomics per expert, and a grid that still fills the chip
    const int rows_per_wave =
        (int)std::max<int64_t>(16, (N + 256 * RT_WAVES - 1) / (256 * RT_WAVES));
    const int64_t rows_per_block = (int64_t)RT_WAVES * rows_per_wave;
    dim3 grid((N + rows_per_block - 1) / rows_per_block);
    auto stream = at::cuda::getCurrentCUDAStream();

#define LAUNCH_RT(T, KV)                                                      \
    hipLaunchKernelGGL((router_topk_kernel<T, KV>), grid, dim3(RT_BLOCK), 0,  \
        stream, reinterpret_cast<const T*>(logits.data_ptr()),                \
        topk_idx.data_ptr<int>(), topk_val.data_ptr<float>(),                 \
        colsum.data_ptr<float>(), count.data_ptr<int>(),                      \
        lse.data_ptr<float>(), N, E, rows_per_wave)

    if (logits.scalar_type() == torch::kFloat) {
        if (k == 1) LAUNCH_RT(float, 1); else LAUNCH_RT(float, 2);
    } else if (logits.scalar_type() == torch::kBFloat16) {
        if (k == 1) LAUNCH_RT(__hip_bfloat16, 1);
        else LAUNCH_RT(__hip_bfloat16, 2);
    } else {
        TORCH_CHECK(false, "router_topk: unsupported dtype");
    }
#undef LAUNCH_RT
    HIP_CHECK_LAUNCH();
    return {topk_idx, topk_val, colsum, count, lse};
}
