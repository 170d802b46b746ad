// Token sampling for gfx950: temperature, top-k and top-p (nucleus) over bf16
// logits [R, V] with per-row parameters read on the device, no host sync, no
// sort.  Semantics (ops/sampling.py states them in full): T == 0 rows take the
// lowest index of the row maximum; other rows keep the logits z >= max(t_k,
// t_p), where t_k is the k-th largest value and t_p the largest value whose
// upper mass reaches top_p of the top-k survivors' mass (ties at a threshold
// are kept), and draw the smallest index whose running kept weight, in
// vocabulary index order, exceeds u * M.
//
// A bf16 row has at most 65 536 distinct values.  key_of() maps the bits to a
// 16-bit key that orders as the values do (-0 folded onto +0), and a
// threshold is found exactly by a two-level 256-bin radix descent: a
// histogram over the high key byte, then one over the low byte inside the bin
// that holds the threshold.  Every keep/drop decision is an integer compare of
// keys.
//
// Masses are fixed point: a weight w = exp2((z - zmax) * log2(e)/T) counts as
// the integer floor(w * 2^40) (V <= 2^20 keeps every sum below 2^61), added
// with integer LDS and global atomics.  Integer addition is associative, so
// every mass, and with it every token, is bit-identical from run to run and
// for every number of splits.  A weight below 2^-40 of the maximum is zero.
//
// Work split: grid (R, S); a row is cut into S contiguous chunks by a host
// plan that depends on shapes only (about TARGET_WGS workgroups, chunks of at
// least MIN_CHUNK elements; `splits` overrides it).  Six launches on the
// current stream share one workspace (RowWs per row):
//   1. max     per-chunk maximum key and its lowest index; clears the row's
//              histograms (plain stores: no memset node in a captured graph)
//   2. hist<0> count and mass per high key byte, all elements
//   3. hist<1> per low byte inside the bin of t_k (rows with top-k on)
//   4. hist<2> per low byte inside the bin of t_p, where that is another bin
//   5. kept    kept mass and last kept index per chunk
//   6. pick    one workgroup per row: scans the S chunk masses, re-reads only
//              the chunk that holds u * M and finds the token by a block
//              prefix scan over packets in index order
// Histograms are per wave in LDS, merged once per workgroup and added to the
// row's table with one global atomic per non-empty bin, so a later pass reads
// 256 entries per row whatever S is.  Each pass derives what it needs from
// the tables at its start (decide()): five 256-wide block scans at the most.
// Greedy rows leave passes 2-5 at once.  Pass 4 is always launched (whether
// any row needs it is known on the device only) and leaves at once where
// top-p is off or t_p shares t_k's bin.
//
// Loads are 16-byte packets (8 bf16 per lane) at 16-byte aligned addresses.
// When V % 8 != 0 a row does not start on such an address: the packets that
// straddle the ends of a chunk are read element by element and masked.
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

#include <algorithm>
#include <cfloat>

#include "common.h"

namespace {

using u64 = unsigned long long;

constexpr int THREADS = 256;
constexpr int NWAVES = THREADS / WAVE_SIZE;
constexpr int BINS = 256;
constexpr int MAX_SPLITS = 64;          // <= WAVE_SIZE: one wave reduces them
constexpr int TARGET_WGS = 512;
constexpr int MIN_CHUNK = 4096;
constexpr int64_t MAX_VOCAB = (int64_t)1 << 20;
constexpr uint32_t KEY_FLOOR = 0x0080;  // the lowest key above -inf
constexpr float FIX_ONE = 1099511627776.f;      // 2^40
constexpr float LOG2E = 1.4426950408889634f;

// one row's workspace; mass/count [0] is the level-1 table, [1] the level-2
// table of t_k's bin, [2] that of t_p's bin
struct RowWs {
    u64 mass[3][BINS];
    u64 chunk_mass[MAX_SPLITS];
    uint32_t count[3][BINS];
    uint32_t max_key[MAX_SPLITS];
    int32_t max_idx[MAX_SPLITS];
    int32_t last_idx[MAX_SPLITS];
};
static_assert(sizeof(RowWs) % 8 == 0, "rows of the workspace are int64 words");

// what decide() leaves in LDS
struct Decision {
    float zmax;
    int arg_idx;            // lowest index of the row maximum
    int bin_a, bin_b;       // the bins of hist<1> and hist<2>, -1: none
    int bin_p;              // the level-1 bin of t_p, -1: top-p off
    uint32_t k_rest;        // rank of t_k inside bin_a
    uint32_t key_k, thr;    // t_k and the final threshold, as keys
    u64 total, mass_above_a, mass_above_p, Mk, M;
    // pick only
    int chunk, token;
    u64 base, tile_total;
};

__device__ __forceinline__ uint32_t key_of(uint16_t b) {
    if (b == 0x8000) b = 0;                         // -0 compares as +0
    return (b & 0x8000) ? (uint16_t)~b : (uint16_t)(b | 0x8000);
}
__device__ __forceinline__ float value_of_key(uint32_t k) {
    const uint32_t b = (k & 0x8000) ? (k & 0x7fff) : (~k & 0xffff);
    return __builtin_bit_cast(float, b << 16);
}
__device__ __forceinline__ float value_of_bits(uint16_t b) {
    return __builtin_bit_cast(float, (uint32_t)b << 16);
}
// the fixed-point weight of logit z; c = log2(e) / T
__device__ __forceinline__ u64 fixed_weight(float z, float zmax, float c) {
    return (u64)(__builtin_amdgcn_exp2f((z - zmax) * c) * FIX_ONE);
}

// Inclusive prefix sum over the 256 threads in thread order; lds holds NWAVES
// words.  All threads call it.
__device__ __forceinline__ u64 block_scan(u64 v, u64* lds) {
    const int lane = threadIdx.x & (WAVE_SIZE - 1);
    const int wave = threadIdx.x / WAVE_SIZE;
#pragma unroll
    for (int off = 1; off < WAVE_SIZE; off <<= 1) {
        const u64 n = __shfl_up(v, off, WAVE_SIZE);
        if (lane >= off) v += n;
    }
    if (lane == WAVE_SIZE - 1) lds[wave] = v;
    __syncthreads();
    u64 add = 0;
    for (int i = 0; i < wave; ++i) add += lds[i];
    __syncthreads();
    return v + add;
}

// Maximum over the workgroup, returned to every thread.
__device__ __forceinline__ u64 block_max(u64 v, u64* lds) {
    const int lane = threadIdx.x & (WAVE_SIZE - 1);
    const int wave = threadIdx.x / WAVE_SIZE;
#pragma unroll
    for (int off = WAVE_SIZE / 2; off > 0; off >>= 1) {
        const u64 n = __shfl_xor(v, off, WAVE_SIZE);
        v = n > v ? n : v;
    }
    if (lane == 0) lds[wave] = v;
    __syncthreads();
    u64 m = lds[0];
    for (int i = 1; i < NWAVES; ++i) m = lds[i] > m ? lds[i] : m;
    __syncthreads();
    return m;
}

// (key, index) packed so that the maximum is the largest key at its lowest
// index
__device__ __forceinline__ u64 pack_max(uint32_t key, int idx) {
    return ((u64)key << 32) | (0xffffffffu - (uint32_t)idx);
}

// mass x reaches the share P of the survivors' mass (and holds something)
__device__ __forceinline__ bool reaches(u64 x, double P) {
    return x > 0 && (double)x >= P;
}

// The chunk [lo, hi) of row `row` as 16-byte packets: packet p covers the
// elements e0 + 8p .. e0 + 8p + 7, with row + e0 16-byte aligned and
// e0 <= lo.
struct Chunk {
    const uint16_t* row;
    int lo, hi, e0, n_packets;
};
__device__ __forceinline__ Chunk make_chunk(const uint16_t* logits, int r,
                                            int V, int s, int chunk) {
    Chunk c;
    c.row = logits + (int64_t)r * V;
    c.lo = s * chunk;
    c.hi = c.lo + chunk < V ? c.lo + chunk : V;
    const int a = (int)((reinterpret_cast<uintptr_t>(c.row) >> 1) & 7);
    c.e0 = c.lo - ((a + c.lo) & 7);
    c.n_packets = (c.hi - c.e0 + 7) >> 3;
    return c;
}
// Loads packet p into b; returns the mask of its elements inside the chunk.
// Only a packet wholly inside is read as one 16-byte load.
__device__ __forceinline__ uint32_t load_packet(const Chunk& c, int p,
                                                uint16_t (&b)[8]) {
    const int e = c.e0 + 8 * p;
    if (e >= c.lo && e + 8 <= c.hi) {
        const uint4 v = *reinterpret_cast<const uint4*>(c.row + e);
        b[0] = v.x & 0xffff; b[1] = v.x >> 16;
        b[2] = v.y & 0xffff; b[3] = v.y >> 16;
        b[4] = v.z & 0xffff; b[5] = v.z >> 16;
        b[6] = v.w & 0xffff; b[7] = v.w >> 16;
        return 0xff;
    }
    uint32_t mask = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        b[i] = 0;
        if (e + i >= c.lo && e + i < c.hi) {
            b[i] = c.row[e + i];
            mask |= 1u << i;
        }
    }
    return mask;
}

// Derives the row's decisions from the workspace into d (LDS), as far as
// `stage` needs them:
//   1  zmax, arg_idx                      (hist<0>, greedy pick)
//   2  + bin_a, k_rest, mass_above_a      (hist<1>)
//   3  + key_k, Mk, bin_p, bin_b          (hist<2>)
//   4  + thr, M                           (kept, pick)
// All 256 threads call it; it ends with a barrier.
__device__ void decide(int stage, const RowWs* w, int S, int V, int k,
                       float p, Decision& d, u64* lds) {
    const int t = threadIdx.x;
    const u64 best = block_max(
        t < S ? pack_max(w->max_key[t], w->max_idx[t]) : 0, lds);
    const bool k_on = k > 0 && k < V;
    const bool p_on = p < 1.f;
    if (t == 0) {
        d.zmax = value_of_key((uint32_t)(best >> 32));
        d.arg_idx = (int)(0xffffffffu - (uint32_t)best);
        d.bin_a = d.bin_b = d.bin_p = -1;
        d.key_k = KEY_FLOOR;
        d.chunk = d.token = -1;
    }
    __syncthreads();
    if (stage == 1) return;

    // level 1: thread t holds bin 255 - t, so that the scan runs downwards
    // from the largest keys
    const int bin = BINS - 1 - t;
    const u64 c1 = w->count[0][bin], m1 = w->mass[0][bin];
    const u64 c1_in = block_scan(c1, lds), m1_in = block_scan(m1, lds);
    if (t == BINS - 1) d.total = d.Mk = m1_in;
    if (k_on && c1_in >= (u64)k && c1_in - c1 < (u64)k) {
        d.bin_a = bin;
        d.k_rest = (uint32_t)((u64)k - (c1_in - c1));
        d.mass_above_a = m1_in - m1;
    }
    __syncthreads();
    if (stage == 2) return;

    const int bin_a = d.bin_a;
    if (bin_a >= 0) {                   // uniform
        const u64 c2 = w->count[1][bin], m2 = w->mass[1][bin];
        const u64 c2_in = block_scan(c2, lds), m2_in = block_scan(m2, lds);
        const u64 rest = d.k_rest;
        if (c2_in >= rest && c2_in - c2 < rest) {
            d.key_k = (uint32_t)(bin_a << 8 | bin);
            d.Mk = d.mass_above_a + m2_in;
        }
        __syncthreads();
    }
    const double P = (double)p * (double)d.Mk;
    if (p_on && reaches(m1_in, P) && !reaches(m1_in - m1, P)) {
        d.bin_p = bin;
        d.mass_above_p = m1_in - m1;
        d.bin_b = bin == bin_a ? -1 : bin;
    }
    __syncthreads();
    if (stage == 3) return;

    const int bin_p = d.bin_p;
    if (t == 0) {
        d.thr = d.key_k;
        d.M = d.Mk;
    }
    __syncthreads();
    if (bin_p >= 0) {                   // uniform
        const u64 m2 = w->mass[bin_p == bin_a ? 1 : 2][bin];
        const u64 above = d.mass_above_p;
        const u64 m2_in = above + block_scan(m2, lds);
        if (reaches(m2_in, P) && !reaches(m2_in - m2, P)) {
            const uint32_t key_p = (uint32_t)(bin_p << 8 | bin);
            // t_p >= t_k by construction; the maximum guards the invariant
            if (key_p >= d.key_k) {
                d.thr = key_p;
                d.M = m2_in;
            }
        }
        __syncthreads();
    }
    if (t == 0 && d.thr < KEY_FLOOR) d.thr = KEY_FLOOR;     // never -inf
    __syncthreads();
}

__device__ __forceinline__ float multiplier(float T) {
    return fminf(LOG2E / T, FLT_MAX);
}

// Pass 1.  Grid (R, S).
__global__ __launch_bounds__(THREADS)
void sample_max_kernel(const uint16_t* __restrict__ logits,
                       RowWs* __restrict__ ws, int V, int chunk) {
    __shared__ u64 lds[NWAVES];
    const int r = blockIdx.x, s = blockIdx.y, S = gridDim.y;
    RowWs* w = ws + r;
    // the S workgroups of a row clear its three tables between them
    u64* mass = &w->mass[0][0];
    uint32_t* count = &w->count[0][0];
    for (int i = s * THREADS + threadIdx.x; i < 3 * BINS; i += S * THREADS) {
        mass[i] = 0;
        count[i] = 0;
    }
    const Chunk c = make_chunk(logits, r, V, s, chunk);
    u64 best = 0;
    for (int p = threadIdx.x; p < c.n_packets; p += THREADS) {
        uint16_t b[8];
        const uint32_t mask = load_packet(c, p, b);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            if (!(mask >> i & 1)) continue;
            const u64 cand = pack_max(key_of(b[i]), c.e0 + 8 * p + i);
            best = cand > best ? cand : best;
        }
    }
    best = block_max(best, lds);
    if (threadIdx.x == 0) {
        w->max_key[s] = (uint32_t)(best >> 32);
        w->max_idx[s] = (int)(0xffffffffu - (uint32_t)best);
    }
}

// Passes 2-4.  LEVEL 0: every element by its high key byte; LEVEL 1 / 2: the
// elements of bin_a / bin_b by their low key byte.  Grid (R, S).
template <int LEVEL>
__global__ __launch_bounds__(THREADS)
void sample_hist_kernel(const uint16_t* __restrict__ logits,
                        const float* __restrict__ temperature,
                        const int* __restrict__ top_k,
                        const float* __restrict__ top_p,
                        RowWs* __restrict__ ws, int V, int chunk) {
    __shared__ u64 lds[NWAVES];
    __shared__ Decision d;
    __shared__ u64 h_mass[NWAVES][BINS];
    __shared__ uint32_t h_count[NWAVES][BINS];
    const int r = blockIdx.x, s = blockIdx.y, S = gridDim.y;
    const float T = temperature[r];
    if (!(T > 0.f)) return;             // greedy row
    RowWs* w = ws + r;
    decide(LEVEL + 1, w, S, V, top_k[r], top_p[r], d, lds);
    const int only = LEVEL == 0 ? 0 : (LEVEL == 1 ? d.bin_a : d.bin_b);
    if (only < 0) return;
    const float zmax = d.zmax, cmul = multiplier(T);

    const int wave = threadIdx.x / WAVE_SIZE;
    for (int i = threadIdx.x; i < NWAVES * BINS; i += THREADS) {
        (&h_mass[0][0])[i] = 0;
        (&h_count[0][0])[i] = 0;
    }
    __syncthreads();

    const Chunk c = make_chunk(logits, r, V, s, chunk);
    for (int p = threadIdx.x; p < c.n_packets; p += THREADS) {
        uint16_t b[8];
        const uint32_t mask = load_packet(c, p, b);
        // neighbours mostly share a bin: runs of one bin make one LDS add
        int run_bin = -1;
        uint32_t run_count = 0;
        u64 run_mass = 0;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            if (!(mask >> i & 1)) continue;
            const uint32_t key = key_of(b[i]);
            if (LEVEL > 0 && (int)(key >> 8) != only) continue;
            const int bin = LEVEL == 0 ? key >> 8 : key & 0xff;
            if (bin != run_bin) {
                if (run_count) {
                    atomicAdd(&h_count[wave][run_bin], run_count);
                    atomicAdd(&h_mass[wave][run_bin], run_mass);
                }
                run_bin = bin;
                run_count = 0;
                run_mass = 0;
            }
            run_count += 1;
            run_mass += fixed_weight(value_of_bits(b[i]), zmax, cmul);
        }
        if (run_count) {
            atomicAdd(&h_count[wave][run_bin], run_count);
            atomicAdd(&h_mass[wave][run_bin], run_mass);
        }
    }
    __syncthreads();

    const int bin = threadIdx.x;
    uint32_t n = 0;
    u64 m = 0;
#pragma unroll
    for (int i = 0; i < NWAVES; ++i) {
        n += h_count[i][bin];
        m += h_mass[i][bin];
    }
    if (n) atomicAdd(&w->count[LEVEL][bin], n);
    if (m) atomicAdd(&w->mass[LEVEL][bin], m);
}

// Pass 5.  Grid (R, S).
__global__ __launch_bounds__(THREADS)
void sample_kept_kernel(const uint16_t* __restrict__ logits,
                        const float* __restrict__ temperature,
                        const int* __restrict__ top_k,
                        const float* __restrict__ top_p,
                        RowWs* __restrict__ ws, int V, int chunk) {
    __shared__ u64 lds[NWAVES];
    __shared__ Decision d;
    const int r = blockIdx.x, s = blockIdx.y, S = gridDim.y;
    const float T = temperature[r];
    if (!(T > 0.f)) return;
    RowWs* w = ws + r;
    decide(4, w, S, V, top_k[r], top_p[r], d, lds);
    const float zmax = d.zmax, cmul = multiplier(T);
    const uint32_t thr = d.thr;

    const Chunk c = make_chunk(logits, r, V, s, chunk);
    u64 mass = 0, last = 0;             // last: kept index + 1
    for (int p = threadIdx.x; p < c.n_packets; p += THREADS) {
        uint16_t b[8];
        const uint32_t mask = load_packet(c, p, b);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            if (!(mask >> i & 1) || key_of(b[i]) < thr) continue;
            mass += fixed_weight(value_of_bits(b[i]), zmax, cmul);
            last = (u64)(c.e0 + 8 * p + i + 1);
        }
    }
    const u64 total = block_scan(mass, lds);
    last = block_max(last, lds);
    if (threadIdx.x == THREADS - 1) {
        w->chunk_mass[s] = total;
        w->last_idx[s] = (int)last - 1;
    }
}

// Pass 6.  Grid (R); S and chunk are those of the other passes.
__global__ __launch_bounds__(THREADS)
void sample_pick_kernel(const uint16_t* __restrict__ logits,
                        const float* __restrict__ u,
                        const float* __restrict__ temperature,
                        const int* __restrict__ top_k,
                        const float* __restrict__ top_p,
                        const RowWs* __restrict__ ws,
                        int64_t* __restrict__ out, int V, int S, int chunk) {
    __shared__ u64 lds[NWAVES];
    __shared__ Decision d;
    const int r = blockIdx.x, t = threadIdx.x;
    const float T = temperature[r];
    const RowWs* w = ws + r;
    if (!(T > 0.f)) {
        decide(1, w, S, V, 0, 1.f, d, lds);
        if (t == 0) out[r] = d.arg_idx;
        return;
    }
    decide(4, w, S, V, top_k[r], top_p[r], d, lds);
    const float zmax = d.zmax, cmul = multiplier(T);
    const uint32_t thr = d.thr;

    // the integer target: the token is the first whose running mass exceeds it
    const double U = (double)u[r] * (double)d.M;
    const u64 target = U >= 1.0 ? (U < 4.0e18 ? (u64)U : ~(u64)0) : 0;

    const u64 cm = t < S ? w->chunk_mass[t] : 0;
    const u64 cm_in = block_scan(cm, lds);
    if (t < S && cm_in > target && cm_in - cm <= target) {
        d.chunk = t;
        d.base = cm_in - cm;
    }
    __syncthreads();
    if (d.chunk >= 0) {
        const Chunk c = make_chunk(logits, r, V, d.chunk, chunk);
        u64 run = d.base;
        for (int p0 = 0; p0 < c.n_packets; p0 += THREADS) {
            const int p = p0 + t;
            u64 wt[8], sum = 0;
#pragma unroll
            for (int i = 0; i < 8; ++i) wt[i] = 0;
            if (p < c.n_packets) {
                uint16_t b[8];
                const uint32_t mask = load_packet(c, p, b);
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    if (!(mask >> i & 1) || key_of(b[i]) < thr) continue;
                    wt[i] = fixed_weight(value_of_bits(b[i]), zmax, cmul);
                    sum += wt[i];
                }
            }
            const u64 in = run + block_scan(sum, lds);
            if (in > target && in - sum <= target) {    // one thread
                u64 acc = in - sum;
                int tok = -1;
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    acc += wt[i];
                    if (tok < 0 && acc > target) tok = c.e0 + 8 * p + i;
                }
                d.token = tok;
            }
            if (t == THREADS - 1) d.tile_total = in;
            __syncthreads();
            if (d.token >= 0) break;
            run = d.tile_total;
            __syncthreads();
        }
    }
    if (t == 0) {
        int tok = d.token;
        if (tok < 0) {                  // u * M not below M: the last kept index
            for (int i = 0; i < S; ++i)
                tok = w->last_idx[i] > tok ? w->last_idx[i] : tok;
        }
        out[r] = tok >= 0 ? tok : d.arg_idx;
    }
}

struct Plan {
    int splits, chunk;
};

// Shapes only.  Chunks are multiples of 8 elements; no chunk is empty.
Plan make_plan(int64_t R, int64_t V, int64_t forced) {
    int64_t s = forced;
    if (s == 0) {
        s = (TARGET_WGS + R - 1) / R;
        s = std::min<int64_t>(s, std::max<int64_t>(1, V / MIN_CHUNK));
        s = std::min<int64_t>(s, MAX_SPLITS);
    }
    const int64_t chunk = ((V + s - 1) / s + 7) / 8 * 8;
    return {(int)((V + chunk - 1) / chunk), (int)chunk};
}

void check_row_param(const char* name, const torch::Tensor& t,
                     torch::ScalarType dtype, const char* dtype_name,
                     int64_t R, const torch::Device& device) {
    TORCH_CHECK(t.is_cuda() && t.device() == device &&
                t.scalar_type() == dtype && t.dim() == 1 && t.size(0) == R &&
                t.is_contiguous(), "sample_logits: ", name,
                " must be a contiguous ", dtype_name, " tensor of ", R,
                " elements on the device of logits");
}

}  // namespace

torch::Tensor sample_logits(torch::Tensor logits, torch::Tensor u,
                            torch::Tensor temperature, torch::Tensor top_k,
                            torch::Tensor top_p, int64_t splits) {
    TORCH_CHECK(logits.is_cuda(), "sample_logits: logits must be on the GPU");
    TORCH_CHECK(logits.scalar_type() == torch::kBFloat16,
                "sample_logits: logits must be bf16");
    TORCH_CHECK(logits.dim() == 2 && logits.is_contiguous(),
                "sample_logits: logits must be a contiguous [R, V] tensor");
    const int64_t R = logits.size(0), V = logits.size(1);
    TORCH_CHECK(V >= 1 && V <= MAX_VOCAB, "sample_logits: V must lie in [1, ",
                MAX_VOCAB, "], got ", V);
    TORCH_CHECK(R < (int64_t)1 << 31, "sample_logits: too many rows");
    TORCH_CHECK(splits >= 0 && splits <= MAX_SPLITS,
                "sample_logits: splits must be 0 (auto) or 1..", MAX_SPLITS,
                ", got ", splits);
    const auto device = logits.device();
    check_row_param("u", u, torch::kFloat, "fp32", R, device);
    check_row_param("temperature", temperature, torch::kFloat, "fp32", R,
                    device);
    check_row_param("top_k", top_k, torch::kInt, "int32", R, device);
    check_row_param("top_p", top_p, torch::kFloat, "fp32", R, device);

    auto out = torch::empty({R}, logits.options().dtype(torch::kLong));
    if (R == 0) return out;
    const Plan plan = make_plan(R, V, splits);
    auto ws_t = torch::empty({R * (int64_t)(sizeof(RowWs) / 8)},
                             logits.options().dtype(torch::kLong));
    RowWs* ws = reinterpret_cast<RowWs*>(ws_t.data_ptr());
    const uint16_t* z = reinterpret_cast<const uint16_t*>(logits.data_ptr());
    const float* T = temperature.data_ptr<float>();
    const int* k = top_k.data_ptr<int>();
    const float* p = top_p.data_ptr<float>();
    const int Vi = (int)V;

    auto stream = at::cuda::getCurrentCUDAStream();
    const dim3 grid((unsigned)R, (unsigned)plan.splits), block(THREADS);
    hipLaunchKernelGGL(sample_max_kernel, grid, block, 0, stream, z, ws, Vi,
                       plan.chunk);
    hipLaunchKernelGGL(sample_hist_kernel<0>, grid, block, 0, stream, z, T, k,
                       p, ws, Vi, plan.chunk);
    hipLaunchKernelGGL(sample_hist_kernel<1>, grid, block, 0, stream, z, T, k,
                       p, ws, Vi, plan.chunk);
    hipLaunchKernelGGL(sample_hist_kernel<2>, grid, block, 0, stream, z, T, k,
                       p, ws, Vi, plan.chunk);
    hipLaunchKernelGGL(sample_kept_kernel, grid, block, 0, stream, z, T, k, p,
                       ws, Vi, plan.chunk);
    hipLaunchKernelGGL(sample_pick_kernel, dim3((unsigned)R), block, 0,
                       stream, z, u.data_ptr<float>(), T, k, p, ws,
                       out.data_ptr<int64_t>(), Vi, plan.splits, plan.chunk);
    HIP_CHECK_LAUNCH();
    return out;
}
