// Device helpers and the split-KV plan shared by the decode attention kernels
// (decode_attention.hip: bf16, contiguous and paged; paged_fp8_attention.hip:
// fp8 pools) and by the fp8 prefill and varlen kernels
// (paged_fp8_prefill_attention.hip, paged_fp8_varlen_attention.hip), the
// split-KV constants of paged_varlen_split_attention.hip and
// paged_fp8_varlen_split_attention.hip, the launcher of the decode combine
// kernel, which lives in decode_attention.hip, and the host plan and combine
// launcher of the ragged split kernels, which live in
// paged_varlen_split_attention.hip and serve its fp8 sibling too.  The designs
// are described in those files' headers.
//
// The device helpers use compiler builtins only (no functions of the HIP
// headers), so that they inline into kernels of any target-feature set.
#pragma once

#include <torch/extension.h>

#include <algorithm>
#include <cfloat>

#include "common.h"

namespace decode_common {

constexpr int TILE = 64;        // keys per workgroup iteration
constexpr int NW = 4;           // waves per workgroup
constexpr int MAX_SPLITS = 64;
constexpr int TARGET_WGS = 1024;
constexpr float LOG2E = 1.4426950408889634f;

__device__ __forceinline__ float bf16_lo(uint32_t w) {
    return __builtin_bit_cast(float, w << 16);
}
__device__ __forceinline__ float bf16_hi(uint32_t w) {
    return __builtin_bit_cast(float, w & 0xffff0000u);
}
// the 8 bf16 of a 16-byte packet
__device__ __forceinline__ void unpack8(const uint4& r, float (&f)[8]) {
    f[0] = bf16_lo(r.x); f[1] = bf16_hi(r.x);
    f[2] = bf16_lo(r.y); f[3] = bf16_hi(r.y);
    f[4] = bf16_lo(r.z); f[5] = bf16_hi(r.z);
    f[6] = bf16_lo(r.w); f[7] = bf16_hi(r.w);
}

// x + (x of the lane that the DPP control selects); all lanes are active
// wherever this is used
template <int CTRL>
__device__ __forceinline__ float dpp_add(float x) {
    return x + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(
                   0, __builtin_bit_cast(int, x), CTRL, 0xf, 0xf, true));
}

// Sum over each aligned group of N (8 or 16) lanes, every lane of the group
// getting the same bits: quad_perm [1,0,3,2] and [2,3,0,1] make the quads
// uniform, row_half_mirror then pairs the two quads of an 8-lane half and
// row_mirror the two halves of a 16-lane row.  DPP rides on the add: no LDS
// traffic, unlike a ds_bpermute shuffle.
template <int N>
__device__ __forceinline__ float group_sum(float x) {
    static_assert(N == 8 || N == 16, "one row is 8 or 16 lanes");
    x = dpp_add<0xB1>(x);
    x = dpp_add<0x4E>(x);
    x = dpp_add<0x141>(x);
    if constexpr (N == 16) x = dpp_add<0x140>(x);
    return x;
}

// max(x, x of the lane that the DPP control selects); whole groups active
template <int CTRL>
__device__ __forceinline__ float dpp_max(float x) {
    return __builtin_fmaxf(
        x, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(
               0, __builtin_bit_cast(int, x), CTRL, 0xf, 0xf, true)));
}

// group_sum's butterfly with max: every lane of an aligned group of N lanes
// gets the group's maximum
template <int N>
__device__ __forceinline__ float group_max(float x) {
    static_assert(N == 8 || N == 16, "one row is 8 or 16 lanes");
    x = dpp_max<0xB1>(x);
    x = dpp_max<0x4E>(x);
    x = dpp_max<0x141>(x);
    if constexpr (N == 16) x = dpp_max<0x140>(x);
    return x;
}

__device__ __forceinline__ int imin(int a, int b) { return a < b ? a : b; }
__device__ __forceinline__ int imax(int a, int b) { return a > b ? a : b; }

// what __syncthreads() is: a workgroup barrier between a release and an
// acquire fence of workgroup scope
__device__ __forceinline__ void block_barrier() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// the query position of batch row b, clamped into the cache
__device__ __forceinline__ int load_pos(const int64_t* __restrict__ pos,
                                        int pos_n, int pos_scalar, int b,
                                        int Skv) {
    int64_t p = pos ? pos[pos_n == 1 ? 0 : b] : (int64_t)pos_scalar;
    p = p < 0 ? 0 : p;
    return (int)(p > Skv - 1 ? Skv - 1 : p);
}

// Merges online-softmax state (m2, l2, a2) into (m, l, a).  Both maxima are
// finite (-FLT_MAX when a state saw no key): the exponents are <= 0 and an
// empty state has l = 0, a = 0, so it contributes nothing.
template <int N>
__device__ __forceinline__ void merge_state(float& m, float& l, float (&a)[N],
                                            float m2, float l2,
                                            const float (&a2)[N]) {
    const float mn = fmaxf(m, m2);
    const float w1 = __builtin_amdgcn_exp2f(m - mn);
    const float w2 = __builtin_amdgcn_exp2f(m2 - mn);
    m = mn;
    l = l * w1 + l2 * w2;
#pragma unroll
    for (int e = 0; e < N; ++e) a[e] = a[e] * w1 + a2[e] * w2;
}

struct DecodePlan {
    int n_splits, chunk;
};

inline int round_up(int64_t x, int64_t to) {
    return (int)((x + to - 1) / to * to);
}

// The plan of decode_attention.hip's file header: shapes only, never the
// position.
inline DecodePlan make_plan(int64_t B, int64_t Hkv, int64_t Skv, int64_t D,
                            int64_t forced) {
    TORCH_CHECK(B > 0 && Hkv > 0 && Skv > 0,
                "decode_attn: B, Hkv and Skv must be positive");
    TORCH_CHECK(D == 64 || D == 128,
                "decode_attn: head dim must be 64 or 128, got ", D);
    TORCH_CHECK(forced >= 0 && forced <= MAX_SPLITS,
                "decode_attn: n_splits must be 0 (auto) or 1..", MAX_SPLITS,
                ", got ", forced);
    TORCH_CHECK(Skv < (int64_t)1 << 30, "decode_attn: Skv too large");
    if (forced > 0)
        return {(int)forced, round_up((Skv + forced - 1) / forced, TILE)};
    int64_t n = (TARGET_WGS + B * Hkv - 1) / (B * Hkv);
    n = std::min<int64_t>(n, std::min<int64_t>(MAX_SPLITS,
                                               (Skv + TILE - 1) / TILE));
    n = std::max<int64_t>(n, 1);
    const int chunk = round_up((Skv + n - 1) / n, TILE);
    return {(int)((Skv + chunk - 1) / chunk), chunk};
}

// Launches decode_attn_combine_kernel<D> (decode_attention.hip) on the
// current stream: grid (H, B), D threads, bf16 output o [B,1,H,D].
void launch_combine(const float* part_acc, const float* part_ml,
                    const int64_t* pos, int pos_n, int pos_scalar,
                    __hip_bfloat16* o, int64_t B, int64_t H, int64_t D,
                    int64_t Skv, const DecodePlan& plan);

// ---- the ragged split-KV kernels (paged_varlen_split_attention.hip and
// paged_fp8_varlen_split_attention.hip): one plan, one combine kernel
constexpr int64_t MAX_WORKSPACE = (int64_t)1 << 31;   // bytes of partials

struct SplitPlan {
    int n_splits, gshift;       // grid z; log2 of the heads sharing an M tile
    int64_t n_slot, ny;         // grid x (tile slots) and y (H >> gshift)
};

// The host plan of paged_varlen_split_attention.hip's file header: shapes
// only.  forced = 0 is the auto plan; `op` names the caller in the errors.
SplitPlan make_split_plan(const char* op, int64_t T, int64_t B, int64_t H,
                          int64_t Hkv, int64_t capacity, int64_t forced);

// Launches paged_varlen_split_combine_kernel<D> (same file) on the current
// stream over the plan's (n_slot, ny) grid: partials indexed (slot, split, y,
// tile row), cu_q read on the device, bf16 output o [T,H,D].
void launch_split_combine(const float* part_acc, const float* part_ml,
                          const int* cu_q, __hip_bfloat16* o,
                          const SplitPlan& plan, int64_t T, int64_t B,
                          int64_t H, int64_t D);

}  // namespace decode_common
