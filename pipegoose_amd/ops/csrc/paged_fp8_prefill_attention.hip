// Paged prefill attention over the fp8 cache for gfx950: the semantics of
// paged_prefill_attn (header of paged_prefill_attention.hip: Sq >= 1 query
// rows at positions start[b] + i, causal cut, ALiBi, GQA, `start` read on the
// device, grid (ceil(Sq/64), H, B) from shapes only, rows outside
// [0, max_pages*PAGE) give zeros) over the storage of paged_fp8_attention.hip:
//
//   k_pool, v_pool   [n_pages, Hkv, PAGE, D]  OCP e4m3fn, one byte per element
//   k_scale, v_scale [n_pages, Hkv, PAGE]     fp32, contiguous, same page ids
//   a value reads back as float(byte) * scale
//
// The MFMA stays bf16 (v_mfma_f32_16x16x32_bf16, 4 waves x 16 query rows,
// 64-key tiles): Q and the softmax weights are bf16/fp32 quantities, and an
// fp8 x fp8 MFMA would quantise both, which the cache format does not ask
// for.  e4m3fn -> bf16 is exact (4 significant bits and exponents 2^-9..2^8
// fit bf16), so the LDS images hold exactly the cached bytes and the scales
// are the only multiplications.
//
// Staging.  A wave stages rows [16w, 16w+16) of a tile: one page, one
// wave-uniform table read, fetched one tile ahead, with the twin's lane map
// (D/8 lanes per row, 8 elements per lane), now 8-byte packets.  The prefetch
// registers hold BYTES while the previous tile is computed, half the twin's
// kr/vr.  store_tile converts once per workgroup: v_cvt_pk_f32_fp8, then the
// upper 16 bits of each fp32 (exact, no rounding step; one v_perm_b32 packs
// two), into the twin's LDS layouts: K row-major on padded rows, V transposed
// with 4-byte row-pair stores.  Converting at fragment-read time would do it
// 4 times, since each of the 4 waves reads the whole tile.
//
// Scales.  The K scales of a wave's 16 rows are 64 contiguous bytes at
// scale[page, hk, in_page], and so are the V scales: lanes 0..15 load the K
// scales and lanes 16..31 the V scales, one 4-byte load per lane with the row
// index clamped to p_max, issued with the tile's byte loads, and store_tile
// puts them into ks_lds[64] / vs_lds[64].  A wave that stages zeros stores
// scale 0.  In the C layout a lane's key column is ns*16 + lcol, fixed per ns,
// so a lane reads 4 K and 4 V scales per tile: the K scale enters the score
// as acc * (scale2 * ks), the product once per ns, and the V scale multiplies
// the softmax weight before its bf16 rounding into p_lds.  l sums the
// UNSCALED fp32 weights.  No dequantised element is ever scaled on its own
// (the decode kernel's rule).
//
// What is never read: the rules of the twin, for bytes AND scales.  p_max is
// the largest in-range position of the workgroup's rows; the key loop runs
// p_max/64 + 1 tiles; row indices are clamped to p_max; a wave whose 16 rows
// start beyond p_max loads nothing; table entries beyond p_max / PAGE are
// never read; every page id is clamped into the pool.  A masked column
// therefore holds the bytes and the scale of row p_max, or zeros and scale 0,
// never a tail value: masking is a select on the score and on the weight,
// and 0 * scale is finite.  No atomics, no split-KV: bit-reproducible.
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

#include <cfloat>
#include <type_traits>

#include "attn_checks.h"
#include "common.h"

// Compiled with the packed-fp32-ops target feature off, for the reason in
// the header of paged_fp8_attention.hip; as there, device code below calls
// compiler builtins only and the device assembly must hold no s_swappc
// (profiles/paged_fp8_prefill_attn.md).
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)
#endif

#include "decode_common.h"

namespace {

using attn_checks::check_operand;
using attn_checks::check_paged_fp8;
using attn_checks::check_position;
using decode_common::block_barrier;
using decode_common::group_max;
using decode_common::group_sum;
using decode_common::imax;
using decode_common::imin;
using decode_common::LOG2E;

using frag_ab = __attribute__((ext_vector_type(8))) __bf16;   // 8 bf16 = 4 VGPR
using frag_cd = __attribute__((ext_vector_type(4))) float;    // 4 fp32
typedef float floatx2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));   // 8 e4m3fn
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int BLOCK_M = 64;   // query rows per workgroup
constexpr int BLOCK_N = 64;   // keys per LDS tile
constexpr int NW = 4;         // waves per workgroup, 16 query rows each
constexpr int PAD = 8;        // bf16 elements (16 B) of row padding in LDS

// bf16(lo) | bf16(hi) << 16 for two fp32 whose low 16 bits are zero (every
// e4m3fn value): bytes 2,3 of each, one v_perm_b32
__device__ __forceinline__ uint32_t pack_bf16(float lo, float hi) {
    return __builtin_amdgcn_perm(__builtin_bit_cast(uint32_t, hi),
                                 __builtin_bit_cast(uint32_t, lo),
                                 0x07060302u);
}

// the 4 e4m3fn of a dword as fp32; fp8 -> fp32 is exact
__device__ __forceinline__ void unpack4_fp8(uint32_t w, float (&f)[4]) {
    const floatx2 a = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, false);
    const floatx2 b = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, true);
    f[0] = a.x; f[1] = a.y; f[2] = b.x; f[3] = b.y;
}

// Pool strides are in bytes (= elements).  Hkv = H / G.
template <int D>
__global__ __launch_bounds__(NW * WAVE_SIZE)
void paged_prefill_attn_fp8_kernel(const __bf16* __restrict__ q,
                                   const uint8_t* __restrict__ k_pool,
                                   const uint8_t* __restrict__ v_pool,
                                   const float* __restrict__ k_scale,
                                   const float* __restrict__ v_scale,
                                   const int* __restrict__ block_table,
                                   int64_t bt_stride,
                                   const float* __restrict__ slopes,
                                   float scale,
                                   const int64_t* __restrict__ start,
                                   int start_n,
                                   __bf16* __restrict__ o,      // [B,Sq,H,D]
                                   int H, int G, int Sq, int capacity,
                                   int n_pages, int page_shift,
                                   int64_t qb, int64_t qh, int64_t qs,
                                   int64_t kpp, int64_t kph, int64_t kps,
                                   int64_t vpp, int64_t vph, int64_t vps) {
    constexpr int DCH = D / 32;     // K-chunks per QK^T mfma row
    constexpr int DSUB = D / 16;    // output d-subtiles
    constexpr int KSTRIDE = D + PAD;
    constexpr int VSTRIDE = BLOCK_N + PAD;
    constexpr int TPR = D / 8;      // 8-byte packets per row
    constexpr int RPL = WAVE_SIZE / TPR;        // rows per wave load
    constexpr int NLK = 16 / RPL;   // K loads per lane and tile
    constexpr int NLV = 8 / RPL;    // V row-pair loads per lane

    // 16-byte packets go in and out of all three
    __shared__ alignas(16) __bf16 k_lds[BLOCK_N * KSTRIDE];
    __shared__ alignas(16) __bf16 vt_lds[D * VSTRIDE];
    __shared__ alignas(16) __bf16 p_lds[NW][16 * VSTRIDE];
    __shared__ float ks_lds[BLOCK_N];
    __shared__ float vs_lds[BLOCK_N];

    const int qblock = __builtin_amdgcn_workgroup_id_x();
    const int h = __builtin_amdgcn_workgroup_id_y();
    const int b = __builtin_amdgcn_workgroup_id_z();
    const int tid = __builtin_amdgcn_workitem_id_x();
    const int wave = tid / WAVE_SIZE;
    const int lane = tid % WAVE_SIZE;
    const int lgrp = lane >> 4;       // 0..3
    const int lcol = lane & 15;       // 0..15
    const int hk = h / G;
    const int Hkv = H / G;

    // capacity and Sq are < 2^30: a start below -2^30 or at or above capacity
    // puts every row out of range either way, and clamped to that interval
    // all the int arithmetic below is exact
    int64_t st64 = start[start_n == 1 ? 0 : b];
    st64 = st64 < -((int64_t)1 << 30) ? -((int64_t)1 << 30) : st64;
    const int st = (int)(st64 > capacity ? capacity : st64);

    const int i0 = qblock * BLOCK_M;                 // first row of the block
    const int i_last = imin(i0 + BLOCK_M, Sq) - 1;   // last REAL row
    const int p_lo = imax(st + i0, 0);
    const int p_max = imin(st + i_last, capacity - 1);

    const int64_t os = (int64_t)H * D;
    __bf16* op = o + ((int64_t)b * Sq * H + h) * D;
    const int wi0 = i0 + wave * 16;                  // this wave's first row

    if (p_lo > p_max) {
        // no row of the block is in range: zeros, and nothing is loaded
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = wi0 + 4 * lgrp + r;
            if (i < Sq) {
#pragma unroll
                for (int ds = 0; ds < DSUB; ++ds)
                    op[i * os + ds * 16 + lcol] = (__bf16)0.f;
            }
        }
        return;
    }

    // the largest in-range position of this wave's rows (-1: none): tiles
    // that start beyond it are wholly masked for the wave
    const int pw_max =
        wi0 < Sq ? imin(st + imin(wi0 + 15, Sq - 1), capacity - 1) : -1;

    frag_ab aQ[DCH];
    {
        // a ragged last block clamps its loads to row Sq-1
        const __bf16* qrow = q + b * qb + h * qh
            + (int64_t)imin(wi0 + lcol, Sq - 1) * qs;
#pragma unroll
        for (int c = 0; c < DCH; ++c)
            aQ[c] = *reinterpret_cast<const frag_ab*>(qrow + c * 32 + 8 * lgrp);
    }
    const float scale2 = scale * LOG2E;              // exp2 domain
    const float slope2 = slopes[h] * LOG2E;

    int prow[4];                                     // position of C-row r
#pragma unroll
    for (int r = 0; r < 4; ++r) prow[r] = st + wi0 + 4 * lgrp + r;

    frag_cd accO[DSUB];
    float m_run[4], l_run[4];
#pragma unroll
    for (int s = 0; s < DSUB; ++s) accO[s] = frag_cd{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int r = 0; r < 4; ++r) { m_run[r] = -FLT_MAX; l_run[r] = 0.f; }

    // ---- staging: this wave moves rows [16*wave, 16*wave+16) of each tile
    const int* bt_row = block_table + b * bt_stride;
    const int page_mask = (1 << page_shift) - 1;
    auto page_of = [&](int row) {
        const int id = bt_row[__builtin_amdgcn_readfirstlane(row) >> page_shift];
        return imin(imax(id, 0), n_pages - 1);
    };
    const uint8_t* kbase = k_pool + hk * kph;
    const uint8_t* vbase = v_pool + hk * vph;
    const int wrow = __builtin_amdgcn_readfirstlane(wave * 16);
    const int k_r = lane / TPR, k_col = (lane % TPR) * 8;   // + it*RPL rows
    // lanes 0..15 carry the K scale of row wrow + lane, lanes 16..31 the V
    // scale of row wrow + lane - 16
    const float* sc_base = lane < 16 ? k_scale : v_scale;

    u32x2 kr[NLK], vr[NLV][2];      // bytes, not bf16
    float sc = 0.f;
    int page = 0;
    if (wrow <= p_max) page = page_of(wrow);

    // fetch the wave's part of the tile at kv0 into registers, then the page
    // id of the NEXT tile if the wave will load there
    auto load_tile = [&](int kv0) {
        const int g0 = kv0 + wrow;
        if (g0 <= p_max) {                           // wave-uniform
            const uint8_t* kpg = kbase + page * kpp + k_col;
            const uint8_t* vpg = vbase + page * vpp + k_col;
#pragma unroll
            for (int it = 0; it < NLK; ++it) {
                // rows past p_max are never loaded: the index is clamped,
                // and stays inside the wave's 16 rows (g0 <= p_max)
                const int jc = imin(g0 + it * RPL + k_r, p_max);
                kr[it] = *reinterpret_cast<const u32x2*>(
                    kpg + (int64_t)(jc & page_mask) * kps);
            }
#pragma unroll
            for (int it = 0; it < NLV; ++it) {
                const int j = g0 + 2 * (it * RPL + k_r);
#pragma unroll
                for (int e = 0; e < 2; ++e)
                    vr[it][e] = *reinterpret_cast<const u32x2*>(
                        vpg + (int64_t)(imin(j + e, p_max) & page_mask) * vps);
            }
            if (lane < 32) {
                // the same clamp: no scale of a row beyond p_max is loaded
                const int jc = imin(g0 + lcol, p_max);
                sc = sc_base[((((int64_t)page * Hkv + hk)) << page_shift)
                             + (jc & page_mask)];
            }
        } else {
            // zeros, not stale LDS: a masked weight is 0 and 0 * NaN is NaN
#pragma unroll
            for (int it = 0; it < NLK; ++it) kr[it] = u32x2{0u, 0u};
#pragma unroll
            for (int it = 0; it < NLV; ++it)
                vr[it][0] = vr[it][1] = u32x2{0u, 0u};
            sc = 0.f;
        }
        if (g0 + BLOCK_N <= p_max) page = page_of(g0 + BLOCK_N);
    };
    // bytes -> bf16, once per workgroup, into the twin's LDS images
    auto store_tile = [&]() {
#pragma unroll
        for (int it = 0; it < NLK; ++it) {
            const int row = wrow + it * RPL + k_r;
            float lo[4], hi[4];
            unpack4_fp8(kr[it].x, lo);
            unpack4_fp8(kr[it].y, hi);
            *reinterpret_cast<u32x4*>(&k_lds[row * KSTRIDE + k_col]) =
                u32x4{pack_bf16(lo[0], lo[1]), pack_bf16(lo[2], lo[3]),
                      pack_bf16(hi[0], hi[1]), pack_bf16(hi[2], hi[3])};
        }
#pragma unroll
        for (int it = 0; it < NLV; ++it) {
            // V transposed; two rows at once -> 4-byte column stores
            const int row = wrow + 2 * (it * RPL + k_r);
            float r0[2][4], r1[2][4];
            unpack4_fp8(vr[it][0].x, r0[0]);
            unpack4_fp8(vr[it][0].y, r0[1]);
            unpack4_fp8(vr[it][1].x, r1[0]);
            unpack4_fp8(vr[it][1].y, r1[1]);
#pragma unroll
            for (int j = 0; j < 8; ++j)
                *reinterpret_cast<uint32_t*>(
                    &vt_lds[(k_col + j) * VSTRIDE + row]) =
                    pack_bf16(r0[j >> 2][j & 3], r1[j >> 2][j & 3]);
        }
        if (lane < 16) ks_lds[wrow + lane] = sc;
        else if (lane < 32) vs_lds[wrow + lane - 16] = sc;
    };

    const int n_tiles = p_max / BLOCK_N + 1;
    load_tile(0);
    for (int t = 0; t < n_tiles; ++t) {
        const int kv0 = t * BLOCK_N;
        block_barrier();               // every wave is done with tile t-1
        store_tile();
        block_barrier();
        if (t + 1 < n_tiles) load_tile(kv0 + BLOCK_N);   // in flight below
        if (kv0 > pw_max) continue;    // wave-uniform: all masked for us

        // S = Q K^T for this wave's rows (16 x 64), exp2 domain, masked; the
        // K scale of column ns*16 + lcol once per ns
        float s_tile[4][4];            // [nsub][reg]
        bool ok[4][4];
        float vs[4];
#pragma unroll
        for (int ns = 0; ns < 4; ++ns) {
            frag_cd acc = frag_cd{0.f, 0.f, 0.f, 0.f};
            __builtin_amdgcn_s_setprio(1);
#pragma unroll
            for (int c = 0; c < DCH; ++c) {
                frag_ab bK = *reinterpret_cast<const frag_ab*>(
                    &k_lds[(ns * 16 + lcol) * KSTRIDE + c * 32 + 8 * lgrp]);
                acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(aQ[c], bK, acc,
                                                              0, 0, 0);
            }
            __builtin_amdgcn_s_setprio(0);
            const float sk = scale2 * ks_lds[ns * 16 + lcol];
            vs[ns] = vs_lds[ns * 16 + lcol];
            const int jk = kv0 + ns * 16 + lcol;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                ok[ns][r] = jk <= prow[r];
                s_tile[ns][r] = __builtin_fmaf(slope2, (float)(jk - prow[r]),
                                               acc[r] * sk);
            }
        }

        // online softmax; masking is a select on the score and the weight
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float mx = -FLT_MAX;
#pragma unroll
            for (int ns = 0; ns < 4; ++ns)
                mx = ok[ns][r] ? __builtin_fmaxf(mx, s_tile[ns][r]) : mx;
            mx = group_max<16>(mx);
            const float m_new = __builtin_fmaxf(m_run[r], mx);
            const float rescale = __builtin_amdgcn_exp2f(m_run[r] - m_new);
            m_run[r] = m_new;
            float ls = 0.f;
#pragma unroll
            for (int ns = 0; ns < 4; ++ns) {
                const float pv = ok[ns][r]
                    ? __builtin_amdgcn_exp2f(s_tile[ns][r] - m_new) : 0.f;
                ls += pv;              // l sums the unscaled weights
                p_lds[wave][(4 * lgrp + r) * VSTRIDE + ns * 16 + lcol] =
                    (__bf16)(pv * vs[ns]);
            }
            ls = group_sum<16>(ls);
            l_run[r] = __builtin_fmaf(l_run[r], rescale, ls);
#pragma unroll
            for (int s = 0; s < DSUB; ++s) accO[s][r] *= rescale;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();   // own-wave P writes before reads
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

        // O += (P * vs) V_bytes  (64 keys in 2 chunks of 32)
#pragma unroll
        for (int kc = 0; kc < 2; ++kc) {
            frag_ab aP = *reinterpret_cast<const frag_ab*>(
                &p_lds[wave][lcol * VSTRIDE + kc * 32 + 8 * lgrp]);
            __builtin_amdgcn_s_setprio(1);
#pragma unroll
            for (int ds = 0; ds < DSUB; ++ds) {
                frag_ab bV = *reinterpret_cast<const frag_ab*>(
                    &vt_lds[(ds * 16 + lcol) * VSTRIDE + kc * 32 + 8 * lgrp]);
                accO[ds] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                    aP, bV, accO[ds], 0, 0, 0);
            }
            __builtin_amdgcn_s_setprio(0);
        }
    }

    // epilogue: real rows only; out-of-range positions give zeros
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int i = wi0 + 4 * lgrp + r;
        if (i >= Sq) continue;
        const bool in_range = prow[r] >= 0 && prow[r] < capacity;
        const float inv_l = in_range ? 1.0f / l_run[r] : 0.f;
        __bf16* orow = op + i * os;
#pragma unroll
        for (int ds = 0; ds < DSUB; ++ds)
            orow[ds * 16 + lcol] =
                (__bf16)(in_range ? accO[ds][r] * inv_l : 0.f);
    }
}

}  // namespace

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

torch::Tensor paged_prefill_attn_fp8(torch::Tensor q, torch::Tensor k_pool,
                                     torch::Tensor v_pool,
                                     torch::Tensor k_scale,
                                     torch::Tensor v_scale,
                                     torch::Tensor block_table,
                                     torch::Tensor slopes, double scale,
                                     torch::Tensor start) {
    const char* op = "paged_prefill_attn_fp8";
    TORCH_CHECK(q.dim() == 4 && q.size(2) >= 1, op,
                ": q must be [B, H, Sq, D] with Sq >= 1");
    const int64_t B = q.size(0), H = q.size(1), Sq = q.size(2), D = q.size(3);
    check_operand(op, "q", q, {B, H, Sq, D});
    const int shift = check_paged_fp8(op, k_pool, v_pool, k_scale, v_scale,
                                      block_table, B, D, q.device());
    const int64_t n_pages = k_pool.size(0), Hkv = k_pool.size(1);
    const int64_t capacity = block_table.size(1) << shift;
    TORCH_CHECK(H % Hkv == 0, op,
                ": q heads must be a multiple of kv heads");
    TORCH_CHECK(slopes.is_cuda() && slopes.scalar_type() == torch::kFloat &&
                slopes.numel() == H && slopes.is_contiguous(), op,
                ": slopes must be ", H, " contiguous fp32 values on the GPU");
    check_position(op, "start", start, B);
    TORCH_CHECK(B > 0 && H > 0 && B <= 65535 && H <= 65535, op,
                ": B and H must fit a grid dimension");
    TORCH_CHECK(Sq < (int64_t)1 << 30, op, ": Sq too large");

    // physically [B, Sq, H, D]: the model's reshape to [B, Sq, H*D] is free
    auto o_phys = torch::empty({B, Sq, H, D}, q.options());
    auto stream = at::cuda::getCurrentCUDAStream();
    auto launch = [&](auto dv_) {
        constexpr int DV = decltype(dv_)::value;
        hipLaunchKernelGGL((paged_prefill_attn_fp8_kernel<DV>),
                           dim3((unsigned)((Sq + BLOCK_M - 1) / BLOCK_M),
                                (unsigned)H, (unsigned)B),
                           dim3(NW * WAVE_SIZE), 0, stream,
                           reinterpret_cast<const __bf16*>(q.data_ptr()),
                           reinterpret_cast<const uint8_t*>(k_pool.data_ptr()),
                           reinterpret_cast<const uint8_t*>(v_pool.data_ptr()),
                           k_scale.data_ptr<float>(),
                           v_scale.data_ptr<float>(),
                           block_table.data_ptr<int>(), block_table.stride(0),
                           slopes.data_ptr<float>(), (float)scale,
                           start.data_ptr<int64_t>(), (int)start.numel(),
                           reinterpret_cast<__bf16*>(o_phys.data_ptr()),
                           (int)H, (int)(H / Hkv), (int)Sq, (int)capacity,
                           (int)n_pages, shift,
                           q.stride(0), q.stride(1), q.stride(2),
                           k_pool.stride(0), k_pool.stride(1), k_pool.stride(2),
                           v_pool.stride(0), v_pool.stride(1),
                           v_pool.stride(2));
    };
    if (D == 64) launch(std::integral_constant<int, 64>{});
    else launch(std::integral_constant<int, 128>{});
    HIP_CHECK_LAUNCH();
    return o_phys.permute({0, 2, 1, 3});
}
