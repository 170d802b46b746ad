// Fused rotary embedding + paged cache write for gfx950: one launch rotates
// the new Q rows, rotates the new K rows and stores them through the block
// table, and stores the new V rows, at positions read on the device.  It
// replaces rope_at_position(q), rope_at_position(k) and paged_kv_write (or
// paged_kv_write_fp8) of the paged LLaMA decode / chunked-prefill step.
//
//   q      [B, H,   S, D] bf16, any strides with d contiguous
//   k_new  [B, Hkv, S, D] bf16, likewise; v_new the same
//   pools  [n_pages, Hkv, PAGE, D] bf16, or e4m3fn with fp32 scales
//          [n_pages, Hkv, PAGE] (the format of paged_fp8_attention.hip)
//   q_rot  physically [B, S, H, D], returned as the [B, H, S, D] view
//
// Paging rules: those of paged_kv_write.  Row s of batch row b sits at
// p = start[b] + s; page ids are clamped into the pool; a row with p outside
// [0, max_pages * PAGE) reads no table entry and writes no pool row and no
// scale, and its q_rot rows are zeros.  The launch plan depends on shapes
// only.
//
// Work split: one workgroup per (b, s) token.  A row of D bf16 is held by a
// group of LG = D/16 lanes; lane `sub` of a group owns the two 16-byte
// packets sub and sub + LG, i.e. the elements d = 8*sub .. 8*sub+7 and their
// partners d + D/2: 8 rotation pairs with both halves in registers, so the
// rotation needs no LDS and no cross-lane traffic.  The pair index depends on
// `sub` alone, so every lane computes its 8 (cos, sin) ONCE, before the row
// loop, and reuses them over all H query rows and Hkv key rows of the token
// (rope.hip evaluates them per head).  The 256/LG groups of the workgroup
// then stride over the H + 2*Hkv rows: Q rows are rotated into q_rot, K rows
// rotated into the pool, V rows copied (bf16) or quantised (fp8).
//
// Angle: angle(p, j) = p * theta^(-2j/D).  freq_tab[j] holds
// theta^(-2j/D) / (2 pi), in revolutions, as an fp32 hi/lo pair computed in
// fp64 on the host.  With pr = p*hi and e = fma(p, hi, -pr) (the exact
// rounding error of pr),
//
//   rev = fract(pr) + (e + p*lo)
//
// is the angle modulo one revolution to about 2^-24 revolutions for every
// p < 2^24 (p itself is exact in fp32), where a plain fp32 p*freq is off by
// 1e-2 rad at p = 2^17.  v_sin_f32 / v_cos_f32 take revolutions.
//
// fp8 pools: the rotated K row is rounded to bf16 first and then quantised
// with the arithmetic of paged_kv_write_fp8 (scale = amax/448, clamp,
// v_cvt_pk_fp8_f32, amax == 0 -> scale 0 and zero bytes), so the cache holds
// what the unfused pair would have cached from the same rotated row.  The
// row amax is a DPP max over the LG lanes of the group; a group works on one
// row at a time and a token is dropped as a whole workgroup, so the DPP max
// only ever runs on whole groups.  The lane with sub == 0 stores the scale.
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

#include <type_traits>

#include "attn_checks.h"
#include "common.h"

// Compiled with the packed-fp32-ops target feature off, as
// paged_fp8_attention.hip (see the note there): device code below calls
// compiler builtins only, never a HIP header function.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)
#endif

#include "decode_common.h"

namespace {

using bf16 = __hip_bfloat16;
using attn_checks::check_operand;
using attn_checks::check_paged;
using attn_checks::check_paged_fp8;
using attn_checks::check_position;
using namespace decode_common;

constexpr int THREADS = 256;
constexpr float E4M3_MAX = 448.0f;

// bf16(lo) | bf16(hi) << 16, round to nearest even
__device__ __forceinline__ uint32_t pack_bf16_rne(float lo, float hi) {
    const uint32_t a = __builtin_bit_cast(uint16_t, (__bf16)lo);
    const uint32_t b = __builtin_bit_cast(uint16_t, (__bf16)hi);
    return a | (b << 16);
}

// members assigned one by one: the vector types' constructors are HIP header
// functions (see the feature note above)
__device__ __forceinline__ uint4 pack8(const float (&f)[8]) {
    uint4 r;
    r.x = pack_bf16_rne(f[0], f[1]);
    r.y = pack_bf16_rne(f[2], f[3]);
    r.z = pack_bf16_rne(f[4], f[5]);
    r.w = pack_bf16_rne(f[6], f[7]);
    return r;
}

// group_max of decode_common.h for the 4- and 8-lane groups of this file
template <int N>
__device__ __forceinline__ float lane_group_max(float x) {
    static_assert(N == 4 || N == 8, "one row is 4 or 8 lanes");
    x = dpp_max<0xB1>(x);
    x = dpp_max<0x4E>(x);
    if constexpr (N == 8) x = dpp_max<0x141>(x);
    return x;
}

__device__ __forceinline__ uint2 to_fp8x8(const float (&f)[8], float inv) {
    float c[8];
#pragma unroll
    for (int e = 0; e < 8; ++e)
        c[e] = __builtin_fminf(__builtin_fmaxf(f[e] * inv, -E4M3_MAX),
                               E4M3_MAX);
    int lo = 0, hi = 0;
    lo = __builtin_amdgcn_cvt_pk_fp8_f32(c[0], c[1], lo, false);
    lo = __builtin_amdgcn_cvt_pk_fp8_f32(c[2], c[3], lo, true);
    hi = __builtin_amdgcn_cvt_pk_fp8_f32(c[4], c[5], hi, false);
    hi = __builtin_amdgcn_cvt_pk_fp8_f32(c[6], c[7], hi, true);
    uint2 r;
    r.x = (uint32_t)lo;
    r.y = (uint32_t)hi;
    return r;
}

// quantise_row of paged_fp8_attention.hip for a lane that holds two packets
// (a, b) of a row spread over LG lanes; returns the row's scale
template <int LG>
__device__ __forceinline__ float quantise_row2(const float (&a)[8],
                                               const float (&b)[8],
                                               uint2& qa, uint2& qb) {
    float amax = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e)
        amax = __builtin_fmaxf(amax, __builtin_fmaxf(__builtin_fabsf(a[e]),
                                                     __builtin_fabsf(b[e])));
    amax = lane_group_max<LG>(amax);
    const float inv = amax > 0.f ? E4M3_MAX / amax : 0.f;
    qa = to_fp8x8(a, inv);
    qb = to_fp8x8(b, inv);
    // a rotated zero row holds -0 where cos < 0: an all-zero row is stored
    // as zero bytes, not as the sign bits
    if (!(amax > 0.f)) qa.x = qa.y = qb.x = qb.y = 0;
    return amax / E4M3_MAX;
}

// y1 = x1*cos - x2*sin, y2 = x2*cos + x1*sin in fp32, rounded once to bf16
__device__ __forceinline__ void rotate(const uint4& r1, const uint4& r2,
                                       const float (&cs)[8],
                                       const float (&sn)[8], uint4& o1,
                                       uint4& o2) {
    float x1[8], x2[8], y1[8], y2[8];
    unpack8(r1, x1);
    unpack8(r2, x2);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        y1[e] = fmaf(x1[e], cs[e], -(x2[e] * sn[e]));
        y2[e] = fmaf(x2[e], cs[e], x1[e] * sn[e]);
    }
    o1 = pack8(y1);
    o2 = pack8(y2);
}

struct RowStrides {
    int64_t b, h, s;
};
struct PoolStrides {
    int64_t p, h, s;
};

// Grid (S, B), 256 threads.  FP8: the pools are bytes (strides in bytes =
// elements) with scales; else bf16 and the scale pointers are unused.
template <int D, bool FP8>
__global__ __launch_bounds__(THREADS)
void paged_rope_write_kernel(const bf16* __restrict__ q,
                             const bf16* __restrict__ k_new,
                             const bf16* __restrict__ v_new,
                             bf16* __restrict__ q_rot,
                             void* __restrict__ k_pool_,
                             void* __restrict__ v_pool_,
                             float* __restrict__ k_scale,
                             float* __restrict__ v_scale,
                             const int* __restrict__ block_table,
                             int64_t bt_stride,
                             const int64_t* __restrict__ start, int start_n,
                             const float* __restrict__ freq_tab,
                             int H, int Hkv, int capacity, int n_pages,
                             int page_shift, RowStrides qs, RowStrides kns,
                             RowStrides vns, PoolStrides kps,
                             PoolStrides vps) {
    constexpr int LG = D / 16;             // lanes per row
    constexpr int NG = THREADS / LG;       // rows per workgroup pass
    constexpr int HALF = D / 2;
    using pool_t = std::conditional_t<FP8, uint8_t, bf16>;
    pool_t* k_pool = static_cast<pool_t*>(k_pool_);
    pool_t* v_pool = static_cast<pool_t*>(v_pool_);

    const int s = blockIdx.x, S = gridDim.x;
    const int b = blockIdx.y;
    const int sub = threadIdx.x % LG;
    const int grp = threadIdx.x / LG;
    const int col = sub * 8;               // first of this lane's 8 pairs

    bf16* qo = q_rot + ((int64_t)b * S + s) * H * D + col;
    const int64_t p = start[start_n == 1 ? 0 : b] + s;
    if (p < 0 || p >= capacity) {          // the whole workgroup: dropped
        uint4 zero;
        zero.x = zero.y = zero.z = zero.w = 0;
        for (int h = grp; h < H; h += NG) {
            *reinterpret_cast<uint4*>(qo + (int64_t)h * D) = zero;
            *reinterpret_cast<uint4*>(qo + (int64_t)h * D + HALF) = zero;
        }
        return;
    }
    const int r = (int)p;
    int page = block_table[b * bt_stride + (r >> page_shift)];
    page = imin(imax(page, 0), n_pages - 1);
    const int in_page = r & ((1 << page_shift) - 1);

    // this lane's 8 (cos, sin), once per token
    float cs[8], sn[8];
    {
        const float pf = (float)r;
        const float4* ft = reinterpret_cast<const float4*>(freq_tab + 2 * col);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float4 t = ft[i];        // (hi, lo) of pairs 2i and 2i + 1
            const float hi[2] = {t.x, t.z}, lo[2] = {t.y, t.w};
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const float pr = pf * hi[j];
                const float err = fmaf(pf, hi[j], -pr);
                const float rev = __builtin_amdgcn_fractf(pr)
                    + fmaf(pf, lo[j], err);
                cs[2 * i + j] = __builtin_amdgcn_cosf(rev);
                sn[2 * i + j] = __builtin_amdgcn_sinf(rev);
            }
        }
    }

    const int n_rows = H + 2 * Hkv;
    for (int row = grp; row < n_rows; row += NG) {     // uniform over a group
        if (row < H) {
            const bf16* src = q + b * qs.b + row * qs.h + s * qs.s + col;
            uint4 o1, o2;
            rotate(*reinterpret_cast<const uint4*>(src),
                   *reinterpret_cast<const uint4*>(src + HALF), cs, sn, o1, o2);
            *reinterpret_cast<uint4*>(qo + (int64_t)row * D) = o1;
            *reinterpret_cast<uint4*>(qo + (int64_t)row * D + HALF) = o2;
            continue;
        }
        const bool is_k = row < H + Hkv;
        const int hk = is_k ? row - H : row - H - Hkv;
        // field by field: a reference picked between the two by-value
        // structs would put them on the stack
        const bf16* src = is_k
            ? k_new + b * kns.b + hk * kns.h + s * kns.s + col
            : v_new + b * vns.b + hk * vns.h + s * vns.s + col;
        uint4 o1 = *reinterpret_cast<const uint4*>(src);
        uint4 o2 = *reinterpret_cast<const uint4*>(src + HALF);
        if (is_k) rotate(o1, o2, cs, sn, o1, o2);
        pool_t* dst = is_k
            ? k_pool + page * kps.p + hk * kps.h + in_page * kps.s + col
            : v_pool + page * vps.p + hk * vps.h + in_page * vps.s + col;
        if constexpr (FP8) {
            float f1[8], f2[8];
            unpack8(o1, f1);
            unpack8(o2, f2);
            uint2 b1, b2;
            const float sc = quantise_row2<LG>(f1, f2, b1, b2);
            *reinterpret_cast<uint2*>(dst) = b1;
            *reinterpret_cast<uint2*>(dst + HALF) = b2;
            if (sub == 0)
                (is_k ? k_scale : v_scale)[
                    (((int64_t)page * Hkv + hk) << page_shift) + in_page] = sc;
        } else {
            *reinterpret_cast<uint4*>(dst) = o1;
            *reinterpret_cast<uint4*>(dst + HALF) = o2;
        }
    }
}

RowStrides row_strides(const torch::Tensor& t) {
    return {t.stride(0), t.stride(1), t.stride(2)};
}
PoolStrides pool_strides(const torch::Tensor& t) {
    return {t.stride(0), t.stride(1), t.stride(2)};
}

}  // namespace

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

namespace {

// The host side of both entry points; k_scale / v_scale are null for bf16
// pools.  freq_tab is the table for (theta, D) that the Python wrapper builds
// and caches; theta itself only names it.
torch::Tensor rope_write(const char* op, const torch::Tensor& q,
                         const torch::Tensor& k_new,
                         const torch::Tensor& v_new,
                         const torch::Tensor& k_pool,
                         const torch::Tensor& v_pool,
                         const torch::Tensor* k_scale,
                         const torch::Tensor* v_scale,
                         const torch::Tensor& block_table,
                         const torch::Tensor& start, double theta,
                         const torch::Tensor& freq_tab) {
    TORCH_CHECK(theta > 0, op, ": theta must be positive, got ", theta);
    TORCH_CHECK(q.dim() == 4 && k_new.dim() == 4 && v_new.dim() == 4, op,
                ": q must be [B, H, S, D], k_new and v_new [B, Hkv, S, D]");
    const int64_t B = q.size(0), H = q.size(1), S = q.size(2), D = q.size(3);
    const int64_t Hkv = k_new.size(1);
    check_operand(op, "q", q, {B, H, S, D});
    check_operand(op, "k_new", k_new, {B, Hkv, S, D});
    check_operand(op, "v_new", v_new, {B, Hkv, S, D});
    const int shift = k_scale
        ? check_paged_fp8(op, k_pool, v_pool, *k_scale, *v_scale, block_table,
                          B, D, q.device())
        : check_paged(op, k_pool, v_pool, block_table, B, D, q.device());
    TORCH_CHECK(k_new.device() == q.device() && v_new.device() == q.device(),
                op, ": all operands must be on the same device");
    TORCH_CHECK(k_pool.size(1) == Hkv, op, ": the pools have ",
                k_pool.size(1), " kv heads, the new rows ", Hkv);
    check_position(op, "start", start, B);
    TORCH_CHECK(freq_tab.is_cuda() && freq_tab.device() == q.device() &&
                freq_tab.scalar_type() == torch::kFloat &&
                freq_tab.is_contiguous() && freq_tab.dim() == 2 &&
                freq_tab.size(0) == D / 2 && freq_tab.size(1) == 2 &&
                reinterpret_cast<uintptr_t>(freq_tab.data_ptr()) % 16 == 0,
                op, ": freq_tab must be a contiguous fp32 [", D / 2,
                ", 2] tensor on the device of q");
    TORCH_CHECK(S < (int64_t)1 << 30 && B <= 65535 && H > 0 &&
                H + 2 * Hkv < (int64_t)1 << 30, op,
                ": B, S or the head counts do not fit one launch");

    // physically [B, S, H, D]: what the attention kernels' epilogues produce
    auto q_phys = torch::empty({B, S, H, D}, q.options());
    if (B * S == 0) return q_phys.permute({0, 2, 1, 3});
    const int64_t capacity = block_table.size(1) << shift;

    auto stream = at::cuda::getCurrentCUDAStream();
    auto launch = [&](auto dv_, auto fp8_) {
        constexpr int DV = decltype(dv_)::value;
        constexpr bool FP8 = decltype(fp8_)::value;
        hipLaunchKernelGGL((paged_rope_write_kernel<DV, FP8>),
                           dim3((unsigned)S, (unsigned)B), dim3(THREADS), 0,
                           stream,
                           reinterpret_cast<const bf16*>(q.data_ptr()),
                           reinterpret_cast<const bf16*>(k_new.data_ptr()),
                           reinterpret_cast<const bf16*>(v_new.data_ptr()),
                           reinterpret_cast<bf16*>(q_phys.data_ptr()),
                           k_pool.data_ptr(), v_pool.data_ptr(),
                           k_scale ? k_scale->data_ptr<float>() : nullptr,
                           v_scale ? v_scale->data_ptr<float>() : nullptr,
                           block_table.data_ptr<int>(), block_table.stride(0),
                           start.data_ptr<int64_t>(), (int)start.numel(),
                           freq_tab.data_ptr<float>(), (int)H, (int)Hkv,
                           (int)capacity, (int)k_pool.size(0), shift,
                           row_strides(q), row_strides(k_new),
                           row_strides(v_new), pool_strides(k_pool),
                           pool_strides(v_pool));
    };
    auto with_d = [&](auto fp8_) {
        if (D == 64) launch(std::integral_constant<int, 64>{}, fp8_);
        else launch(std::integral_constant<int, 128>{}, fp8_);
    };
    if (k_scale) with_d(std::true_type{});
    else with_d(std::false_type{});
    HIP_CHECK_LAUNCH();
    return q_phys.permute({0, 2, 1, 3});
}

}  // namespace

torch::Tensor paged_rope_write(torch::Tensor q, torch::Tensor k_new,
                               torch::Tensor v_new, torch::Tensor k_pool,
                               torch::Tensor v_pool,
                               torch::Tensor block_table, torch::Tensor start,
                               double theta, torch::Tensor freq_tab) {
    return rope_write("paged_rope_write", q, k_new, v_new, k_pool, v_pool,
                      nullptr, nullptr, block_table, start, theta, freq_tab);
}

torch::Tensor paged_rope_write_fp8(torch::Tensor q, torch::Tensor k_new,
                                   torch::Tensor v_new, torch::Tensor k_pool,
                                   torch::Tensor v_pool,
                                   torch::Tensor k_scale,
                                   torch::Tensor v_scale,
                                   torch::Tensor block_table,
                                   torch::Tensor start, double theta,
                                   torch::Tensor freq_tab) {
    return rope_write("paged_rope_write_fp8", q, k_new, v_new, k_pool, v_pool,
                      &k_scale, &v_scale, block_table, start, theta,
                      freq_tab);
}
