// MoE dispatch/combine around the grouped expert GEMMs (gfx950, bf16).
//
// N tokens, router fan-out k, S = N*k slots; slot s = t*k + j is token t's
// j-th choice.  The routing plan sorts the KEPT slots by (local expert,
// slot) -- a stable counting sort, the order torch.argsort(stable=True)
// gives -- into the first M rows of an S-row buffer:
//
//   offsets[e]      first row of local expert e, offsets[E] = M
//   row_of_slot[s]  row of slot s, -1 when the slot was dropped
//   slot_of_row[r]  slot at row r, -1 for the dead rows r >= M
//
// Nothing is read back by the host, nothing is atomic, no block waits for
// another: the plan is three launches on one stream,
//
//   1. per-chunk, per-expert histogram (chunk = 256 threads x 4 slots; the
//      lanes of a wave that share an expert find each other with one
//      __ballot per id bit)
//   2. one block scans the [chunks, E] table into chunk bases and offsets
//   3. pass 1 again: wave-local rank + prefix inside the chunk (LDS) +
//      chunk base = row; writes both maps
//
// and the four row movers go through those maps only:
//
//   permute_fwd  xs[r]  = x[slot_of_row[r] / k]            dead rows: zeros
//   permute_bwd  dx[t]  = sum_j dxs[row_of_slot[t*k+j]]    fp32, ascending j
//   combine_fwd  out[t] = sum_j g[s] * ys[row_of_slot[s]]  fp32, ascending j
//   combine_bwd  dys[r] = g[s] * dout[t],  dgate[s] = <dout[t], ys[r]>
//
// Rows are whole contiguous bf16 rows with H % 8 == 0: every access is a
// 16-byte packet per lane, a wave owns ROWS_PER_WAVE destination rows and
// keeps that many loads in flight per packet column.  Every index read out
// of a plan tensor is checked against its range and a bad entry is treated
// as dropped, so a caller's mistake gives wrong numbers, not a fault.
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

#include "common.h"

namespace {

constexpr int MAX_EXPERTS = 64;
constexpr int NTHREADS = 256;                     // 4 waves
constexpr int NWAVES = NTHREADS / WAVE_SIZE;
constexpr int SLOTS_PER_THREAD = 4;
constexpr int CHUNK = NTHREADS * SLOTS_PER_THREAD;  // 1024 slots
constexpr int NSEG = SLOTS_PER_THREAD * NWAVES;   // wave-passes per chunk
constexpr int ROWS_PER_WAVE = 4;
constexpr int ROWS_PER_BLOCK = ROWS_PER_WAVE * NWAVES;

// ------------------------------------------------------------------- plan
template <typename WT>
__device__ __forceinline__ bool weight_positive(const WT* w, int64_t i) {
    return to_float(w[i]) > 0.f;  // false for NaN
}

// Local expert of slot s, or -1 when the slot is dropped.
template <typename WT>
__device__ __forceinline__ int slot_expert(const int64_t* __restrict__ order,
                                           const WT* __restrict__ weight,
                                           int64_t s, int64_t S, int k,
                                           int64_t e0, int E, int64_t E_tot) {
    if (s >= S) return -1;
    const int64_t id = order[s];
    if (id < e0 || id >= e0 + (int64_t)E) return -1;
    if (weight != nullptr) {
        // range first: a bad id is a dropped slot, never an index
        if (id < 0 || id >= E_tot) return -1;
        if (!weight_positive(weight, (s / k) * E_tot + id)) return -1;
    }
    return (int)(id - e0);
}

// Passes 1 (WRITE = false: hist[chunk][e]) and 3 (WRITE = true: the maps).
// Slot of (pass i, thread tid) is chunk*CHUNK + i*NTHREADS + tid, so the
// (pass, wave) segments of a chunk are in slot order.
template <typename WT, bool WRITE>
__global__ __launch_bounds__(NTHREADS)
void route_chunk_kernel(const int64_t* __restrict__ order,
                        const WT* __restrict__ weight,
                        int* __restrict__ hist,            // [chunks, E]
                        const int* __restrict__ base,      // [chunks, E]
                        const int* __restrict__ offsets,   // [E+1]
                        int* __restrict__ row_of_slot,
                        int* __restrict__ slot_of_row,
                        int64_t S, int k, int64_t e0, int E, int64_t E_tot) {
    __shared__ int cnt[NSEG][MAX_EXPERTS];
    const int tid = threadIdx.x;
    const int wave = tid / WAVE_SIZE, lane = tid % WAVE_SIZE;
    const int64_t chunk = blockIdx.x;

    for (int i = tid; i < NSEG * MAX_EXPERTS; i += NTHREADS)
        (&cnt[0][0])[i] = 0;
    __syncthreads();

    int le[SLOTS_PER_THREAD], rank[SLOTS_PER_THREAD];
    const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
    for (int i = 0; i < SLOTS_PER_THREAD; ++i) {
        const int64_t s = chunk * CHUNK + (int64_t)i * NTHREADS + tid;
        le[i] = slot_expert(order, weight, s, S, k, e0, E, E_tot);
        // lanes of this wave with the same expert (wave-uniform control flow)
        unsigned long long same = __ballot(le[i] >= 0);
#pragma unroll
        for (int b = 0; b < 6; ++b) {
            const bool bit = (le[i] >> b) & 1;
            const unsigned long long bal = __ballot(bit);
            same &= bit ? bal : ~bal;
        }
        rank[i] = __popcll(same & below);
        if (le[i] >= 0 && rank[i] == 0)
            cnt[i * NWAVES + wave][le[i]] = __popcll(same);
    }
    __syncthreads();

    // exclusive scan over the chunk's segments, one expert per thread
    if (tid < MAX_EXPERTS) {
        int run = 0;
#pragma unroll
        for (int g = 0; g < NSEG; ++g) {
            const int c = cnt[g][tid];
            cnt[g][tid] = run;
            run += c;
        }
        if (!WRITE && tid < E) hist[chunk * E + tid] = run;
    }
    if (!WRITE) return;
    __syncthreads();

    const int M = offsets[E];
#pragma unroll
    for (int i = 0; i < SLOTS_PER_THREAD; ++i) {
        const int64_t s = chunk * CHUNK + (int64_t)i * NTHREADS + tid;
        if (s >= S) continue;
        int row = -1;
        if (le[i] >= 0) {
            row = base[chunk * E + le[i]] + cnt[i * NWAVES + wave][le[i]] +
                  rank[i];
            if (row < 0 || row >= S) row = -1;
            else slot_of_row[row] = (int)s;
        }
        row_of_slot[s] = row;
        // rows M..S-1 are nobody's: this block marks the ones it indexes
        if (s >= M) slot_of_row[s] = -1;
    }
}

// Pass 2: hist[chunks, E] -> base[chunks, E] (first row of expert e's slots
// of chunk c) and offsets[E+1].  One block; thread (p, e) owns a contiguous
// range of chunks for expert e and walks it serially, twice.  Sized for the
// banks this serves (S up to ~10^6 slots: at most a few hundred chunks per
// thread); it stays correct for any S < 2^31 but a thread then walks up to
// chunks * epad / 256 entries, so far larger S wants a multi-block scan.
__global__ __launch_bounds__(NTHREADS)
void route_scan_kernel(const int* __restrict__ hist, int* __restrict__ base,
                       int* __restrict__ offsets, int64_t chunks, int E,
                       int epad) {
    __shared__ int part[NTHREADS];
    __shared__ int off[MAX_EXPERTS + 1];
    const int tid = threadIdx.x;
    const int e = tid % epad, p = tid / epad, P = NTHREADS / epad;
    const int64_t per = (chunks + P - 1) / P;
    const int64_t c0 = per * p < chunks ? per * p : chunks;
    const int64_t c1 = c0 + per < chunks ? c0 + per : chunks;

    int sum = 0;
    if (e < E)
        for (int64_t c = c0; c < c1; ++c) sum += hist[c * E + e];
    part[tid] = sum;
    __syncthreads();
    if (p == 0) {  // exclusive scan over the parts of expert e
        int run = 0;
        for (int q = 0; q < P; ++q) {
            const int v = part[q * epad + e];
            part[q * epad + e] = run;
            run += v;
        }
        off[e + 1] = run;  // total of expert e (epad <= MAX_EXPERTS)
    }
    __syncthreads();
    if (tid == 0) {
        off[0] = 0;
        for (int i = 0; i < E; ++i) off[i + 1] += off[i];
    }
    __syncthreads();
    if (tid <= E) offsets[tid] = off[tid];
    if (e < E) {
        int run = off[e] + part[tid];
        for (int64_t c = c0; c < c1; ++c) {
            const int v = hist[c * E + e];
            base[c * E + e] = run;
            run += v;
        }
    }
}

// ------------------------------------------------------------- row movers
__device__ __forceinline__ void unpack8(const uint4& v, float* f) {
    const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        f[2 * i] = __uint_as_float(w[i] << 16);
        f[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
    }
}

__device__ __forceinline__ unsigned pack2(float lo, float hi) {
    // __float2bfloat16 rounds to nearest even
    return (unsigned)__bfloat16_as_ushort(__float2bfloat16(lo)) |
           ((unsigned)__bfloat16_as_ushort(__float2bfloat16(hi)) << 16);
}

__device__ __forceinline__ uint4 pack8(const float* f) {
    return make_uint4(pack2(f[0], f[1]), pack2(f[2], f[3]),
                      pack2(f[4], f[5]), pack2(f[6], f[7]));
}

// xs[r] = x[slot_of_row[r] / k]; dead rows are zeros.
__global__ __launch_bounds__(NTHREADS)
void permute_fwd_kernel(const uint4* __restrict__ x,
                        const int* __restrict__ slot_of_row,
                        uint4* __restrict__ xs, int64_t S, int k, int HP) {
    const int wave = threadIdx.x / WAVE_SIZE, lane = threadIdx.x % WAVE_SIZE;
    const int64_t r0 = (int64_t)blockIdx.x * ROWS_PER_BLOCK +
                       wave * ROWS_PER_WAVE;
    int64_t tok[ROWS_PER_WAVE];
#pragma unroll
    for (int i = 0; i < ROWS_PER_WAVE; ++i) {
        const int64_t r = r0 + i;
        const int64_t s = r < S ? slot_of_row[r] : -1;
        tok[i] = (s >= 0 && s < S) ? s / k : -1;  // s < N*k, so tok < N
    }
    for (int p = lane; p < HP; p += WAVE_SIZE) {
        uint4 v[ROWS_PER_WAVE];
#pragma unroll
        for (int i = 0; i < ROWS_PER_WAVE; ++i) {
            v[i] = make_uint4(0, 0, 0, 0);
            if (tok[i] >= 0) v[i] = x[tok[i] * HP + p];
        }
#pragma unroll
        for (int i = 0; i < ROWS_PER_WAVE; ++i)
            if (r0 + i < S) xs[(r0 + i) * HP + p] = v[i];
    }
}

// out[t] = sum_j g[t*k+j] * src[row_of_slot[t*k+j]] over the kept slots,
// accumulated in fp32 in ascending j and rounded once.  GATED = false is
// the plain sum (permute backward, or an unweighted combine).
template <bool GATED>
__global__ __launch_bounds__(NTHREADS)
void gather_sum_kernel(const uint4* __restrict__ src,
                       const float* __restrict__ gates,
                       const int* __restrict__ row_of_slot,
                       uint4* __restrict__ out, int64_t N, int64_t S, int k,
                       int HP) {
    const int wave = threadIdx.x / WAVE_SIZE, lane = threadIdx.x % WAVE_SIZE;
    const int64_t t0 = (int64_t)blockIdx.x * ROWS_PER_BLOCK +
                       wave * ROWS_PER_WAVE;
    for (int p = lane; p < HP; p += WAVE_SIZE) {
        float acc[ROWS_PER_WAVE][8];
#pragma unroll
        for (int i = 0; i < ROWS_PER_WAVE; ++i)
#pragma unroll
            for (int h = 0; h < 8; ++h) acc[i][h] = 0.f;
        for (int j = 0; j < k; ++j) {
            uint4 v[ROWS_PER_WAVE];
            float g[ROWS_PER_WAVE];
            bool live[ROWS_PER_WAVE];
#pragma unroll
            for (int i = 0; i < ROWS_PER_WAVE; ++i) {
                const int64_t s = (t0 + i) * k + j;
                const int64_t r = t0 + i < N ? row_of_slot[s] : -1;
                live[i] = r >= 0 && r < S;
                g[i] = 1.f;
                if (live[i]) {
                    v[i] = src[r * HP + p];
                    if (GATED) g[i] = gates[s];
                }
            }
#pragma unroll
            for (int i = 0; i < ROWS_PER_WAVE; ++i) {
                if (!live[i]) continue;
                float f[8];
                unpack8(v[i], f);
#pragma unroll
                for (int h = 0; h < 8; ++h) {
                    if (GATED) acc[i][h] += g[i] * f[h];
                    else acc[i][h] += f[h];
                }
            }
        }
#pragma unroll
        for (int i = 0; i < ROWS_PER_WAVE; ++i)
            if (t0 + i < N) out[(t0 + i) * HP + p] = pack8(acc[i]);
    }
}

// For a live row r (slot s, token t): dys[r] = bf16(g[s] * dout[t]) and
// dgate[s] = sum_h dout[t,h] * ys[r,h], both from one read of dout[t].
// Dead rows of dys are zeros; dgate arrives zero-filled.
template <bool GATED, bool DGATE>
__global__ __launch_bounds__(NTHREADS)
void combine_bwd_kernel(const uint4* __restrict__ dout,
                        const uint4* __restrict__ ys,
                        const float* __restrict__ gates,
                        const int* __restrict__ slot_of_row,
                        uint4* __restrict__ dys, float* __restrict__ dgate,
                        int64_t S, int k, int HP) {
    const int wave = threadIdx.x / WAVE_SIZE, lane = threadIdx.x % WAVE_SIZE;
    const int64_t r0 = (int64_t)blockIdx.x * ROWS_PER_BLOCK +
                       wave * ROWS_PER_WAVE;
    int64_t slot[ROWS_PER_WAVE];
    float g[ROWS_PER_WAVE], dot[ROWS_PER_WAVE];
#pragma unroll
    for (int i = 0; i < ROWS_PER_WAVE; ++i) {
        const int64_t r = r0 + i;
        const int64_t s = r < S ? slot_of_row[r] : -1;
        slot[i] = (s >= 0 && s < S) ? s : -1;
        g[i] = (GATED && slot[i] >= 0) ? gates[slot[i]] : 1.f;
        dot[i] = 0.f;
    }
    for (int p = lane; p < HP; p += WAVE_SIZE) {
        uint4 d[ROWS_PER_WAVE], y[ROWS_PER_WAVE];
#pragma unroll
        for (int i = 0; i < ROWS_PER_WAVE; ++i) {
            if (slot[i] < 0) continue;
            d[i] = dout[(slot[i] / k) * HP + p];
            if (DGATE) y[i] = ys[(r0 + i) * HP + p];
        }
#pragma unroll
        for (int i = 0; i < ROWS_PER_WAVE; ++i) {
            if (r0 + i >= S) continue;
            uint4 o = make_uint4(0, 0, 0, 0);
            if (slot[i] >= 0) {
                float fd[8];
                unpack8(d[i], fd);
                if (DGATE) {
                    float fy[8];
                    unpack8(y[i], fy);
#pragma unroll
                    for (int h = 0; h < 8; ++h) dot[i] += fd[h] * fy[h];
                }
                if (GATED) {
#pragma unroll
                    for (int h = 0; h < 8; ++h) fd[h] *= g[i];
                    o = pack8(fd);
                } else {
                    o = d[i];
                }
            }
            dys[(r0 + i) * HP + p] = o;
        }
    }
    if (DGATE) {
#pragma unroll
        for (int i = 0; i < ROWS_PER_WAVE; ++i) {
            const float tot = wave_reduce_sum(dot[i]);  // wave-uniform loop
            if (lane == 0 && slot[i] >= 0) dgate[slot[i]] = tot;
        }
    }
}

// ------------------------------------------------------------ host checks
void check_rows(const torch::Tensor& t, const char* name) {
    TORCH_CHECK(t.is_cuda() && t.dim() == 2 &&
                    t.scalar_type() == torch::kBFloat16 && t.is_contiguous(),
                "moe_permute: ", name,
                " must be a contiguous 2-D bf16 device tensor");
    TORCH_CHECK(t.size(1) % 8 == 0 && t.size(1) > 0, "moe_permute: ", name,
                " needs a row length that is a multiple of 8, got ",
                t.size(1));
}

void check_map(const torch::Tensor& m, const torch::Tensor& like, int64_t S,
               const char* name) {
    TORCH_CHECK(m.is_cuda() && m.device() == like.device() &&
                    m.scalar_type() == torch::kInt32 && m.dim() == 1 &&
                    m.is_contiguous() && m.numel() == S,
                "moe_permute: ", name, " must be a contiguous int32 [", S,
                "] vector on the operands' device");
}

void check_gates(const c10::optional<torch::Tensor>& g,
                 const torch::Tensor& like, int64_t S) {
    if (!g.has_value()) return;
    TORCH_CHECK(g->is_cuda() && g->device() == like.device() &&
                    g->scalar_type() == torch::kFloat && g->dim() == 1 &&
                    g->is_contiguous() && g->numel() == S,
                "moe_permute: gates must be a contiguous fp32 [", S,
                "] vector on the operands' device");
}

int64_t slots_of(int64_t N, int64_t k) {
    TORCH_CHECK(N >= 0 && k >= 1, "moe_permute: need N >= 0 and k >= 1");
    TORCH_CHECK(N * k < (int64_t)1 << 31, "moe_permute: N*k must be < 2^31");
    return N * k;
}

unsigned row_blocks(int64_t rows) {
    return (unsigned)((rows + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK);
}

inline const uint4* cptr(const torch::Tensor& t) {
    return reinterpret_cast<const uint4*>(t.data_ptr());
}
inline uint4* mptr(torch::Tensor& t) {
    return reinterpret_cast<uint4*>(t.data_ptr());
}

}  // namespace

std::vector<torch::Tensor> moe_route_plan(torch::Tensor order,
                                          c10::optional<torch::Tensor> weight,
                                          int64_t e0, int64_t E) {
    TORCH_CHECK(order.is_cuda() && order.dim() == 2 &&
                    order.scalar_type() == torch::kInt64 &&
                    order.is_contiguous(),
                "moe_route_plan: order must be a contiguous int64 [N,k] "
                "device tensor");
    TORCH_CHECK(E >= 1 && E <= MAX_EXPERTS, "moe_route_plan: 1 <= E <= ",
                MAX_EXPERTS, " local experts, got ", E);
    const int64_t N = order.size(0), k = order.size(1);
    const int64_t S = slots_of(N, k);
    int64_t E_tot = 0;
    bool w_bf16 = false;
    if (weight.has_value()) {
        TORCH_CHECK(weight->is_cuda() && weight->device() == order.device() &&
                        weight->dim() == 2 && weight->size(0) == N &&
                        weight->is_contiguous(),
                    "moe_route_plan: weight must be a contiguous [N,E_tot] "
                    "tensor on order's device");
        TORCH_CHECK(weight->scalar_type() == torch::kBFloat16 ||
                        weight->scalar_type() == torch::kFloat,
                    "moe_route_plan: weight must be bf16 or fp32");
        E_tot = weight->size(1);
        w_bf16 = weight->scalar_type() == torch::kBFloat16;
    }
    auto iopt = order.options().dtype(torch::kInt32);
    auto offsets = torch::empty({E + 1}, iopt);
    auto row_of_slot = torch::empty({S}, iopt);
    auto slot_of_row = torch::empty({S}, iopt);
    if (S == 0) {
        offsets.zero_();
        return {offsets, row_of_slot, slot_of_row};
    }
    const int64_t chunks = (S + CHUNK - 1) / CHUNK;
    auto table = torch::empty({2, chunks, E}, iopt);  // hist, base
    int* hist = table.data_ptr<int>();
    int* base = hist + chunks * E;
    int epad = 1;
    while (epad < E) epad <<= 1;
    auto stream = at::cuda::getCurrentCUDAStream();
    const void* wptr = weight.has_value() ? weight->data_ptr() : nullptr;
#define LAUNCH(WT, WRITE)                                                     \
    hipLaunchKernelGGL((route_chunk_kernel<WT, WRITE>),                       \
        dim3((unsigned)chunks), dim3(NTHREADS), 0, stream,                    \
        order.data_ptr<int64_t>(), reinterpret_cast<const WT*>(wptr), hist,   \
        base, offsets.data_ptr<int>(), row_of_slot.data_ptr<int>(),           \
        slot_of_row.data_ptr<int>(), S, (int)k, e0, (int)E, E_tot)
    if (w_bf16) LAUNCH(__hip_bfloat16, false);
    else LAUNCH(float, false);
    HIP_CHECK_LAUNCH();
    hipLaunchKernelGGL(route_scan_kernel, dim3(1), dim3(NTHREADS), 0, stream,
                       hist, base, offsets.data_ptr<int>(), chunks, (int)E,
                       epad);
    HIP_CHECK_LAUNCH();
    if (w_bf16) LAUNCH(__hip_bfloat16, true);
    else LAUNCH(float, true);
#undef LAUNCH
    HIP_CHECK_LAUNCH();
    return {offsets, row_of_slot, slot_of_row};
}

torch::Tensor moe_permute_fwd(torch::Tensor x, torch::Tensor slot_of_row,
                              int64_t k) {
    check_rows(x, "x");
    const int64_t N = x.size(0), H = x.size(1), S = slots_of(N, k);
    check_map(slot_of_row, x, S, "slot_of_row");
    auto xs = torch::empty({S, H}, x.options());
    if (S == 0) return xs;
    hipLaunchKernelGGL(permute_fwd_kernel, dim3(row_blocks(S)),
                       dim3(NTHREADS), 0, at::cuda::getCurrentCUDAStream(),
                       cptr(x), slot_of_row.data_ptr<int>(), mptr(xs), S,
                       (int)k, (int)(H / 8));
    HIP_CHECK_LAUNCH();
    return xs;
}

torch::Tensor moe_permute_bwd(torch::Tensor dxs, torch::Tensor row_of_slot,
                              int64_t N, int64_t k) {
    check_rows(dxs, "dxs");
    const int64_t H = dxs.size(1), S = slots_of(N, k);
    TORCH_CHECK(dxs.size(0) == S, "moe_permute_bwd: dxs must have N*k rows");
    check_map(row_of_slot, dxs, S, "row_of_slot");
    auto dx = torch::empty({N, H}, dxs.options());
    if (N == 0) return dx;
    hipLaunchKernelGGL((gather_sum_kernel<false>), dim3(row_blocks(N)),
                       dim3(NTHREADS), 0, at::cuda::getCurrentCUDAStream(),
                       cptr(dxs), nullptr, row_of_slot.data_ptr<int>(),
                       mptr(dx), N, S, (int)k, (int)(H / 8));
    HIP_CHECK_LAUNCH();
    return dx;
}

torch::Tensor moe_combine_fwd(torch::Tensor ys,
                              c10::optional<torch::Tensor> gates,
                              torch::Tensor row_of_slot, int64_t N,
                              int64_t k) {
    check_rows(ys, "ys");
    const int64_t H = ys.size(1), S = slots_of(N, k);
    TORCH_CHECK(ys.size(0) == S, "moe_combine_fwd: ys must have N*k rows");
    check_map(row_of_slot, ys, S, "row_of_slot");
    check_gates(gates, ys, S);
    auto out = torch::empty({N, H}, ys.options());
    if (N == 0) return out;
    auto stream = at::cuda::getCurrentCUDAStream();
    if (gates.has_value()) {
        hipLaunchKernelGGL((gather_sum_kernel<true>), dim3(row_blocks(N)),
                           dim3(NTHREADS), 0, stream, cptr(ys),
                           gates->data_ptr<float>(),
                           row_of_slot.data_ptr<int>(), mptr(out), N, S,
                           (int)k, (int)(H / 8));
    } else {
        hipLaunchKernelGGL((gather_sum_kernel<false>), dim3(row_blocks(N)),
                           dim3(NTHREADS), 0, stream, cptr(ys), nullptr,
                           row_of_slot.data_ptr<int>(), mptr(out), N, S,
                           (int)k, (int)(H / 8));
    }
    HIP_CHECK_LAUNCH();
    return out;
}

std::vector<torch::Tensor> moe_combine_bwd(torch::Tensor dout,
                                           torch::Tensor ys,
                                           c10::optional<torch::Tensor> gates,
                                           torch::Tensor slot_of_row,
                                           int64_t k, bool want_dgate) {
    check_rows(dout, "dout");
    check_rows(ys, "ys");
    const int64_t N = dout.size(0), H = dout.size(1), S = slots_of(N, k);
    TORCH_CHECK(ys.device() == dout.device() && ys.size(0) == S &&
                    ys.size(1) == H,
                "moe_combine_bwd: ys must be [N*k,H] on dout's device");
    check_map(slot_of_row, dout, S, "slot_of_row");
    check_gates(gates, dout, S);
    auto fopt = dout.options().dtype(torch::kFloat);
    auto dys = torch::empty({S, H}, dout.options());
    auto dgate = want_dgate ? torch::zeros({S}, fopt)
                            : torch::empty({0}, fopt);
    if (S == 0) return {dys, dgate};
    auto stream = at::cuda::getCurrentCUDAStream();
    const float* gp = gates.has_value() ? gates->data_ptr<float>() : nullptr;
#define LAUNCH(GATED, DGATE)                                                  \
    hipLaunchKernelGGL((combine_bwd_kernel<GATED, DGATE>),                    \
        dim3(row_blocks(S)), dim3(NTHREADS), 0, stream, cptr(dout),           \
        cptr(ys), gp, slot_of_row.data_ptr<int>(), mptr(dys),                 \
        want_dgate ? dgate.data_ptr<float>() : nullptr, S, (int)k,            \
        (int)(H / 8))
    if (gates.has_value()) {
        if (want_dgate) LAUNCH(true, true);
        else LAUNCH(true, false);
    } else {
        if (want_dgate) LAUNCH(false, true);
        else LAUNCH(false, false);
    }
#undef LAUNCH
    HIP_CHECK_LAUNCH();
    return {dys, dgate};
}
