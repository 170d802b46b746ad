// Split-KV ragged-batch paged attention over the fp8 cache for gfx950: the
// semantics and storage of paged_varlen_attn_fp8
// (paged_fp8_varlen_attention.hip) with the work split and plan of
// paged_varlen_split_attn (paged_varlen_split_attention.hip).  Both headers
// carry over: q [T,H,D] bf16 token-packed; k_pool, v_pool [n_pages, Hkv,
// PAGE, D] e4m3fn bytes; k_scale, v_scale [n_pages, Hkv, PAGE] fp32, a value
// reads back as float(byte) * scale; block_table [B, max_pages]; slopes;
// cu_q int32 [B+1] and start int64 READ ON THE DEVICE; padding rows and rows
// outside [0, max_pages*PAGE) give exact zeros; every page id and every cu_q
// value clamped; no byte, scale or table entry past the largest visible
// position read.  n_splits (0 = auto, 1..MAX_SPLITS forced); o [T,H,D] bf16.
// No atomics: results are bit-reproducible for fixed inputs and plan.
//
// Work split: grid (N_slot, H/gp, n_splits), M tile = 64/gp tokens x the gp
// heads of one kv head, slots found by the in-kernel cu_q scan.  The host plan
// (shapes only) and the combine kernel are the bf16 split kernel's, through
// decode_common::make_split_plan and decode_common::launch_split_combine:
// one definition, in paged_varlen_split_attention.hip, so the two cannot
// drift.  Only host code was exported there; that file's kernels and their
// recorded resource numbers are unchanged.  The cu_q scan and the padding
// zeroing are repeated here in raw-builtin form, as in
// paged_fp8_varlen_attention.hip and for its reason (no HIP header function
// inlines into device code built with packed-fp32-ops off).
//
// Device plan, per tile: chunk = round_up(ceil((p_max+1)/n_splits), 64),
// split s owns keys [k_lo, k_end] = [s*chunk, min((s+1)*chunk, p_max+1) - 1].
// A split with s*chunk > p_max is dead: it writes the empty state (m =
// -FLT_MAX, l = 0) for the tile's real rows and touches no K, V, scale or
// table entry.  fp32 unnormalised partials (m, l, acc[D], exp2 domain) go to
// a torch::empty workspace indexed (slot, split, y, tile row); the combine
// kernel merges them in split order and selects on l == 0.  With n_splits ==
// 1 the kernel writes o itself: no workspace, no second launch.
//
// Masking.  Row indices (bytes and scales) are clamped to k_end, not to
// p_max.  The chunk is a multiple of the 64-key tile, so k_end is either the
// last key of a key tile or p_max: a key past k_end inside a tile is past
// p_max, hence past every row's position, and is masked by the causal test
// alone, exactly as in the bf16 split kernel.  A masked column holds the
// bytes and scale of row k_end, or zeros and scale 0, never a tail value;
// masking is a select on the score and on the weight.
//
// Scales, both bodies: the K scale enters the score as acc * (scale2 * ks),
// the V scale multiplies the softmax weight before its single bf16 rounding
// into P, l sums the UNSCALED fp32 weights.  The two bodies round the same
// quantities the same number of times.
//
// Shared-tile body: the key loop of paged_varlen_attn_fp8 over [k_lo, k_end].
// Each wave stages rows [16w, 16w+16) of a 64-key tile, prefetched a tile
// ahead as BYTES in 8-byte packets, the 16 K scales and 16 V scales of those
// rows riding in lanes 0..15 and 16..31; bytes -> bf16 once per workgroup
// (v_cvt_pk_f32_fp8 + v_perm_b32) on the way into the K and V^T LDS images,
// scales through ks_lds / vs_lds.  A wave whose staged rows start past k_end
// stages zero bytes and scale 0.
//
// Short body, for tiles with n_tok * gp <= 16 (workgroup-uniform: decode
// rows).  The 4 waves serve the same 16 rows, each against its own 16-key
// slice of every 64-key tile (16-aligned, inside one page for every allowed
// PAGE: one wave-uniform table lookup):
//   - K bytes go from HBM straight to the MFMA B operand, never through LDS:
//     lane = key row lcol, 8 contiguous bytes at c*32 + 8*lgrp (half the bf16
//     body's load width), converted in registers; each element is used once,
//     so nothing is converted twice;
//   - both scales of a key are per lane: column lcol of the C layout is key
//     g0 + lcol, so each lane loads that key's K scale and V scale (index
//     clamped to k_end), one 4-byte load each, no LDS, no cross-lane traffic;
//   - V bytes are converted and written transposed into the wave's private
//     LDS slice, P next to it; wave-level synchronisation only in the loop;
//   - PV is the 16x16x32 MFMA with the upper 16 k-lanes zero;
//   - the next slice's bytes and its two scales are in flight during the
//     current slice's maths; a slice that starts past k_end is not loaded and
//     ends the loop;
//   - per-wave (m, l, accO) merge once at the end through LDS, in wave order,
//     and all 256 threads write the partial, or o when n_splits == 1.
// short_body = false (binding argument) runs every tile through the
// shared-tile body.  profiles/paged_fp8_mixed_attn.md has the measurements of
// both bodies.
//
// Resources (hipcc -O3 --offload-arch=gfx950
// -Rpass-analysis=kernel-resource-usage), n_splits == 1 / n_splits > 1:
//   D = 64 : 122 / 121 VGPRs + 16 AGPRs, 100 / 93 SGPRs, 28160 B LDS,
//            3 waves/SIMD
//   D = 128: 161 / 159 VGPRs + 32 AGPRs, 100 / 93 SGPRs, 45568 B LDS,
//            2 waves/SIMD
// no scratch in any of them, 0 s_swappc and 0 v_pk_*_f32 in the device
// assembly: the waves/SIMD of paged_varlen_attn_fp8 (120 / 154 VGPRs).  The
// same compile of paged_varlen_split_attention.hip gives that header's
// numbers for its three kernels, unchanged by the export.
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

#include <cfloat>
#include <type_traits>

#include "attn_checks.h"
#include "common.h"

// Compiled with the packed-fp32-ops target feature off, for the reason in
// the header of paged_fp8_attention.hip; as there, device code below calls
// compiler builtins only.
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

constexpr int BLOCK_M = 64;   // (token, head) rows per workgroup
constexpr int BLOCK_N = 64;   // keys per key tile
constexpr int NW = 4;         // waves per workgroup
constexpr int PAD = 8;        // bf16 elements (16 B) of row padding in LDS
constexpr int SV = 16 + PAD;  // row stride of a wave's private 16-key slices
constexpr int MAX_SEQS = 1024;
constexpr int MAX_TOKENS = 1 << 20;

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

// the 8 e4m3fn of a packet as 8 bf16, exact
__device__ __forceinline__ u32x4 fp8x8_to_bf16(u32x2 w) {
    float lo[4], hi[4];
    unpack4_fp8(w.x, lo);
    unpack4_fp8(w.y, hi);
    return u32x4{pack_bf16(lo[0], lo[1]), pack_bf16(lo[2], lo[3]),
                 pack_bf16(hi[0], hi[1]), pack_bf16(hi[2], hi[3])};
}

// x of lane `src` of the wave (ds_bpermute); every lane is active wherever
// this is used, and a src below 0 is never consumed
__device__ __forceinline__ int lane_read(int x, int src) {
    return __builtin_amdgcn_ds_bpermute(src << 2, x);
}

// own-wave LDS writes before own-wave reads (and the reverse)
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <int D>
struct Lds {
    static constexpr int KSTRIDE = D + PAD;
    static constexpr int VSTRIDE = BLOCK_N + PAD;
    // K, V^T and P images (bf16), then ks_lds[64] and vs_lds[64]
    static constexpr int IMAGES =
        (BLOCK_N * KSTRIDE + D * VSTRIDE + NW * 16 * VSTRIDE) * 2;
    static constexpr int SHARED = IMAGES + 2 * BLOCK_N * 4;
    static constexpr int SLICE = (D + 16) * SV;            // bf16 per wave
    static constexpr int MSTRIDE = D + 2;                  // acc, m, l
    static constexpr int MERGE = NW * 16 * MSTRIDE * 4;
    static_assert(NW * SLICE * 2 <= SHARED && MERGE <= SHARED, "LDS reuse");
};

// Pool strides are in bytes (= elements).  Hkv = H / G.  n_wg, ny and nsp are
// the grid's extents.
template <int D, bool SPLIT>
__global__ __launch_bounds__(NW * WAVE_SIZE)
void paged_varlen_split_attn_fp8_kernel(
        const __bf16* __restrict__ q, const uint8_t* __restrict__ k_pool,
        const uint8_t* __restrict__ v_pool, const float* __restrict__ k_scale,
        const float* __restrict__ v_scale,
        const int* __restrict__ block_table, int64_t bt_stride,
        const float* __restrict__ slopes, float scale,
        const int* __restrict__ cu_q, const int64_t* __restrict__ start,
        int start_n,
        __bf16* __restrict__ o,               // [T,H,D]
        float* __restrict__ part_acc,         // [slot,split,y,64,D]
        float* __restrict__ part_ml,          // [slot,split,y,64,2]
        int T, int B, int H, int G, int gshift, int short_body,
        int n_wg, int ny, int nsp,
        int capacity, int n_pages, int page_shift,
        int64_t qt, int64_t qh,
        int64_t kpp, int64_t kph, int64_t kps,
        int64_t vpp, int64_t vph, int64_t vps) {
    constexpr int DCH = D / 32;     // K-chunks per QK^T mfma row
    constexpr int DSUB = D / 16;    // output d-subtiles
    constexpr int KSTRIDE = Lds<D>::KSTRIDE;
    constexpr int VSTRIDE = Lds<D>::VSTRIDE;
    constexpr int MSTRIDE = Lds<D>::MSTRIDE;
    constexpr int TPR = D / 8;      // 8-byte packets per row
    constexpr int RPL = WAVE_SIZE / TPR;        // rows per wave load
    constexpr int NLK = 16 / RPL;   // K loads per lane and tile
    constexpr int NLV = 8 / RPL;    // V row-pair loads per lane

    __shared__ alignas(16) char lds_raw[Lds<D>::SHARED];

    const int wg = __builtin_amdgcn_workgroup_id_x();
    const int wy = __builtin_amdgcn_workgroup_id_y();
    const int split = __builtin_amdgcn_workgroup_id_z();
    const int tid = __builtin_amdgcn_workitem_id_x();
    const int wave = tid / WAVE_SIZE;
    const int lane = tid % WAVE_SIZE;
    const int lgrp = lane >> 4;       // 0..3
    const int lcol = lane & 15;       // 0..15
    const int gmask = (1 << gshift) - 1;
    const int tpt_shift = 6 - gshift;           // TPT = 64 >> gshift tokens
    const int TPT = 1 << tpt_shift;
    const int h0 = wy << gshift;                // first head of the tile
    const int hk = h0 / G;
    const int Hkv = H / G;
    const int64_t os = (int64_t)H * D;

    auto cu = [&](int i) { return imin(imax(cu_q[i], 0), T); };

    // ---- which (sequence, tile) is this slot?  Every wave scans alone: the
    // results are wave-uniform and equal in all four
    int total = 0, seq = -1, tile = 0;
    for (int base = 0; base < B; base += WAVE_SIZE) {
        const int b = base + lane;
        int n = 0;
        if (b < B) n = (imax(cu(b + 1) - cu(b), 0) + TPT - 1) >> tpt_shift;
        int incl = n;                           // inclusive prefix sum
#pragma unroll
        for (int off = 1; off < WAVE_SIZE; off <<= 1) {
            const int up = lane_read(incl, lane - off);
            if (lane >= off) incl += up;
        }
        incl += total;
        const uint64_t hit = __builtin_amdgcn_ballot_w64(incl > wg);
        if (seq < 0 && hit != 0) {              // wave-uniform
            const int l = __builtin_ctzll(hit);
            seq = base + l;
            tile = wg - lane_read(incl - n, l);
        }
        total = lane_read(incl, WAVE_SIZE - 1);
    }
    seq = __builtin_amdgcn_readfirstlane(seq);
    tile = __builtin_amdgcn_readfirstlane(tile);
    total = __builtin_amdgcn_readfirstlane(total);

    if (seq < 0) {
        // a surplus slot: the zeros of the padding rows, strided over the
        // surplus slots, each thread one 16-byte packet at a time.  SPLIT:
        // the combine kernel writes them
        if constexpr (!SPLIT) {
            const int n_surplus = n_wg - total;
            const int row = tid >> 2;           // tile row 0..63
            const int head = h0 + (row & gmask);
            for (int64_t t = (int64_t)cu(B) + (int64_t)(wg - total) * TPT
                     + (row >> gshift);
                 t < T; t += (int64_t)n_surplus * TPT) {
                __bf16* orow = o + t * os + (int64_t)head * D;
                for (int c = (tid & 3) * 8; c < D; c += 32)
                    *reinterpret_cast<u32x4*>(orow + c) = u32x4{0u, 0u, 0u, 0u};
            }
        }
        return;
    }

    const int c0 = cu(seq);
    const int len = imax(cu(seq + 1) - c0, 0);
    const int i0 = tile << tpt_shift;           // first row of the tile in seq
    const int n_tok = imin(TPT, len - i0);      // real tokens here, >= 1
    const int tok0 = c0 + i0;                   // packed index, tok0+n_tok <= T

    // capacity and T are < 2^30: a start below -2^30 or at or above capacity
    // puts every row out of range either way, and clamped to that interval
    // all the int arithmetic below is exact
    int64_t st64 = start[start_n == 1 ? 0 : seq];
    st64 = st64 < -((int64_t)1 << 30) ? -((int64_t)1 << 30) : st64;
    const int st = (int)(st64 > capacity ? capacity : st64);

    const int p_lo = imax(st + i0, 0);
    const int p_max = imin(st + i0 + n_tok - 1, capacity - 1);

    // this workgroup's rows of the partial workspace
    const int64_t wsrow = (((int64_t)wg * nsp + split) * ny + wy) * BLOCK_M;

    // the device plan: keys [k_lo, k_end] of this split (file header)
    int k_lo = 0, k_end = p_max;
    bool dead = p_lo > p_max;       // no row of the tile is in range
    if (SPLIT && !dead) {
        const int chunk =
            ((p_max + nsp) / nsp + BLOCK_N - 1) & ~(BLOCK_N - 1);
        k_lo = split * chunk;       // < n_keys + 65 * nsp: no overflow
        k_end = imin(k_lo + chunk, p_max + 1) - 1;
        dead = k_lo > p_max;
    }
    if (dead) {
        // nothing is loaded: the empty state, or the zeros themselves
        if constexpr (SPLIT) {
            if (tid < BLOCK_M && (tid >> gshift) < n_tok) {
                part_ml[2 * (wsrow + tid)] = -FLT_MAX;
                part_ml[2 * (wsrow + tid) + 1] = 0.f;
            }
        } else {
            const int row = tid >> 2;
            const int ti = row >> gshift;
            if (ti < n_tok) {
                __bf16* orow = o + (int64_t)imin(tok0 + ti, T - 1) * os
                    + (int64_t)(h0 + (row & gmask)) * D;
                for (int c = (tid & 3) * 8; c < D; c += 32)
                    *reinterpret_cast<u32x4*>(orow + c) = u32x4{0u, 0u, 0u, 0u};
            }
        }
        return;
    }

    const float scale2 = scale * LOG2E;              // exp2 domain
    const int* bt_row = block_table + seq * bt_stride;
    const int page_mask = (1 << page_shift) - 1;
    auto page_of = [&](int row) {
        const int id = bt_row[__builtin_amdgcn_readfirstlane(row) >> page_shift];
        return imin(imax(id, 0), n_pages - 1);
    };
    // the scales of a page's rows for this kv head
    auto scale_row = [&](int page) {
        return ((int64_t)page * Hkv + hk) << page_shift;
    };
    const uint8_t* kbase = k_pool + hk * kph;
    const uint8_t* vbase = v_pool + hk * vph;
    const int wrow = __builtin_amdgcn_readfirstlane(wave * 16);
    const int k_r = lane / TPR, k_col = (lane % TPR) * 8;   // + it*RPL rows

    frag_cd accO[DSUB];
    float m_run[4], l_run[4];
#pragma unroll
    for (int s = 0; s < DSUB; ++s) accO[s] = frag_cd{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int r = 0; r < 4; ++r) { m_run[r] = -FLT_MAX; l_run[r] = 0.f; }

    if (short_body && (n_tok << gshift) <= 16) {
        // ================= short tile: 4 waves x 16 keys, the same 16 rows
        __bf16* vts = reinterpret_cast<__bf16*>(lds_raw) + wave * Lds<D>::SLICE;
        __bf16* ps = vts + D * SV;

        frag_ab aQ[DCH];
        {
            const int tg =
                imin(imax(tok0 + imin(lcol >> gshift, n_tok - 1), 0), T - 1);
            const __bf16* qrow =
                q + tg * qt + (int64_t)(h0 + (lcol & gmask)) * qh;
#pragma unroll
            for (int c = 0; c < DCH; ++c)
                aQ[c] = *reinterpret_cast<const frag_ab*>(qrow + c * 32 + 8 * lgrp);
        }
        int prow[4];
        float slope2[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = 4 * lgrp + r;
            prow[r] = st + i0 + (row >> gshift);
            slope2[r] = slopes[h0 + (row & gmask)] * LOG2E;
        }

        // the wave's 16 keys of the tile at kv0: K bytes in B-operand layout,
        // V bytes in row pairs, and this lane's key's two scales; a slice
        // that starts past k_end is not loaded (and ends the loop)
        u32x2 kn[DCH], vn[NLV][2];
        float ksn = 0.f, vsn = 0.f;
        auto load_slice = [&](int kv0) {
            const int g0 = kv0 + wrow;
            if (g0 > k_end) return;                     // wave-uniform
            const int page = page_of(g0);
            // rows past k_end are never loaded: clamped, inside the slice
            const int jc = imin(g0 + lcol, k_end) & page_mask;
            const uint8_t* kpg = kbase + page * kpp + (int64_t)jc * kps
                + 8 * lgrp;
#pragma unroll
            for (int c = 0; c < DCH; ++c)
                kn[c] = *reinterpret_cast<const u32x2*>(kpg + c * 32);
            const int64_t srow = scale_row(page) + jc;
            ksn = k_scale[srow];
            vsn = v_scale[srow];
            const uint8_t* vpg = vbase + page * vpp + k_col;
#pragma unroll
            for (int it = 0; it < NLV; ++it) {
                const int j = g0 + 2 * (it * RPL + k_r);
#pragma unroll
                for (int e = 0; e < 2; ++e)
                    vn[it][e] = *reinterpret_cast<const u32x2*>(
                        vpg + (int64_t)(imin(j + e, k_end) & page_mask) * vps);
            }
        };

        load_slice(k_lo);
        for (int kv0 = k_lo; kv0 + wrow <= k_end; kv0 += BLOCK_N) {
            u32x2 kc[DCH];
#pragma unroll
            for (int c = 0; c < DCH; ++c) kc[c] = kn[c];
            const float sk = scale2 * ksn, vs = vsn;
#pragma unroll
            for (int it = 0; it < NLV; ++it) {
                // V converted and transposed; two rows at once -> 4-byte
                // column stores
                const int row = 2 * (it * RPL + k_r);
                float r0[2][4], r1[2][4];
                unpack4_fp8(vn[it][0].x, r0[0]);
                unpack4_fp8(vn[it][0].y, r0[1]);
                unpack4_fp8(vn[it][1].x, r1[0]);
                unpack4_fp8(vn[it][1].y, r1[1]);
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    *reinterpret_cast<uint32_t*>(
                        &vts[(k_col + j) * SV + row]) =
                        pack_bf16(r0[j >> 2][j & 3], r1[j >> 2][j & 3]);
            }
            load_slice(kv0 + BLOCK_N);                  // in flight below

            // S = Q K^T: the bytes become the B operand in registers
            frag_cd acc = frag_cd{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int c = 0; c < DCH; ++c)
                acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                    aQ[c], __builtin_bit_cast(frag_ab, fp8x8_to_bf16(kc[c])),
                    acc, 0, 0, 0);
            const int jk = kv0 + wrow + lcol;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const bool ok = jk <= prow[r];
                const float s = __builtin_fmaf(
                    slope2[r], (float)(jk - prow[r]), acc[r] * sk);
                const float mx = group_max<16>(ok ? s : -FLT_MAX);
                const float m_new = __builtin_fmaxf(m_run[r], mx);
                const float rescale = __builtin_amdgcn_exp2f(m_run[r] - m_new);
                m_run[r] = m_new;
                const float pv = ok ? __builtin_amdgcn_exp2f(s - m_new) : 0.f;
                ps[(4 * lgrp + r) * SV + lcol] = (__bf16)(pv * vs);
                // l sums the unscaled weights
                l_run[r] = __builtin_fmaf(l_run[r], rescale, group_sum<16>(pv));
#pragma unroll
                for (int s2 = 0; s2 < DSUB; ++s2) accO[s2][r] *= rescale;
            }
            wave_sync();            // own-wave V^T and P writes before reads

            // O += (P * vs) V_bytes: k-lanes 0..15 are the keys, 16..31 zeros
            frag_ab aP = frag_ab{};
            if (lgrp < 2)
                aP = *reinterpret_cast<const frag_ab*>(&ps[lcol * SV + 8 * lgrp]);
#pragma unroll
            for (int ds = 0; ds < DSUB; ++ds) {
                frag_ab bV = frag_ab{};
                if (lgrp < 2)
                    bV = *reinterpret_cast<const frag_ab*>(
                        &vts[(ds * 16 + lcol) * SV + 8 * lgrp]);
                accO[ds] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                    aP, bV, accO[ds], 0, 0, 0);
            }
            wave_sync();            // reads before the next slice's writes
        }

        // the four waves' states -> LDS -> merged in wave order by all
        float* sm = reinterpret_cast<float*>(lds_raw);
        block_barrier();            // every wave has left its slices
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float* srow = sm + (wave * 16 + 4 * lgrp + r) * MSTRIDE;
#pragma unroll
            for (int ds = 0; ds < DSUB; ++ds) srow[ds * 16 + lcol] = accO[ds][r];
            if (lcol == 0) { srow[D] = m_run[r]; srow[D + 1] = l_run[r]; }
        }
        block_barrier();
        const int row = tid >> 4, cl = tid & 15;    // 16 rows x 16 columns
        float m = -FLT_MAX, l = 0.f, a[DSUB];
#pragma unroll
        for (int ds = 0; ds < DSUB; ++ds) a[ds] = 0.f;
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            const float* srow = sm + (w * 16 + row) * MSTRIDE;
            const float m2 = srow[D], l2 = srow[D + 1];
            if (l2 > 0.f) {
                const float mn = __builtin_fmaxf(m, m2);
                const float w1 = __builtin_amdgcn_exp2f(m - mn);
                const float w2 = __builtin_amdgcn_exp2f(m2 - mn);
                m = mn;
                l = l * w1 + l2 * w2;
#pragma unroll
                for (int ds = 0; ds < DSUB; ++ds)
                    a[ds] = a[ds] * w1 + srow[ds * 16 + cl] * w2;
            }
        }
        const int ti = row >> gshift;
        if (ti >= n_tok) return;
        const int p = st + i0 + ti;
        const bool live = p >= 0 && p < capacity && l > 0.f;
        if constexpr (SPLIT) {
            if (cl == 0) {
                part_ml[2 * (wsrow + row)] = live ? m : -FLT_MAX;
                part_ml[2 * (wsrow + row) + 1] = live ? l : 0.f;
            }
            if (live) {
                float* prow_ = part_acc + (wsrow + row) * D;
#pragma unroll
                for (int ds = 0; ds < DSUB; ++ds) prow_[ds * 16 + cl] = a[ds];
            }
        } else {
            const float inv_l = live ? 1.0f / l : 0.f;
            __bf16* orow = o + (int64_t)imin(tok0 + ti, T - 1) * os
                + (int64_t)(h0 + (row & gmask)) * D;
#pragma unroll
            for (int ds = 0; ds < DSUB; ++ds)
                orow[ds * 16 + cl] = (__bf16)(live ? a[ds] * inv_l : 0.f);
        }
        return;
    }

    // ======== shared tile: paged_varlen_attn_fp8's loop over [k_lo, k_end]
    __bf16* k_lds = reinterpret_cast<__bf16*>(lds_raw);
    __bf16* vt_lds = k_lds + BLOCK_N * KSTRIDE;
    __bf16* p_lds = vt_lds + D * VSTRIDE + wave * 16 * VSTRIDE;
    float* ks_lds = reinterpret_cast<float*>(lds_raw + Lds<D>::IMAGES);
    float* vs_lds = ks_lds + BLOCK_N;
    const int wr0 = wave * 16;                  // this wave's first tile row

    // the largest in-range position of this wave's real rows (-1: none):
    // key tiles that start beyond it are wholly masked for the wave
    const int wt0 = wr0 >> gshift, wt1 = (wr0 + 15) >> gshift;
    const int pw_max = wt0 < n_tok
        ? imin(st + i0 + imin(wt1, n_tok - 1), capacity - 1) : -1;

    frag_ab aQ[DCH];
    {
        // A-fragment row = lcol; rows past the last real token re-read it
        const int row = wr0 + lcol;
        const int tg =
            imin(imax(tok0 + imin(row >> gshift, n_tok - 1), 0), T - 1);
        const __bf16* qrow = q + tg * qt + (int64_t)(h0 + (row & gmask)) * qh;
#pragma unroll
        for (int c = 0; c < DCH; ++c)
            aQ[c] = *reinterpret_cast<const frag_ab*>(qrow + c * 32 + 8 * lgrp);
    }
    int prow[4];                                     // position of C-row r
    float slope2[4];                                 // its head's slope
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = wr0 + 4 * lgrp + r;
        prow[r] = st + i0 + (row >> gshift);
        slope2[r] = slopes[h0 + (row & gmask)] * LOG2E;
    }

    // ---- staging: this wave moves rows [16*wave, 16*wave+16) of each tile;
    // lanes 0..15 carry the K scale of row wrow + lane, lanes 16..31 the V
    // scale of row wrow + lane - 16
    const float* sc_base = lane < 16 ? k_scale : v_scale;
    u32x2 kr[NLK], vr[NLV][2];      // bytes, not bf16
    float sc = 0.f;
    int page = 0;
    if (k_lo + wrow <= k_end) page = page_of(k_lo + wrow);

    // fetch the wave's part of the tile at kv0 into registers, then the page
    // id of the NEXT tile if the wave will load there
    auto load_tile = [&](int kv0) {
        const int g0 = kv0 + wrow;
        if (g0 <= k_end) {                           // wave-uniform
            const uint8_t* kpg = kbase + page * kpp + k_col;
            const uint8_t* vpg = vbase + page * vpp + k_col;
#pragma unroll
            for (int it = 0; it < NLK; ++it) {
                // rows past k_end are never loaded: the index is clamped,
                // and stays inside the wave's 16 rows (g0 <= k_end)
                const int jc = imin(g0 + it * RPL + k_r, k_end);
                kr[it] = *reinterpret_cast<const u32x2*>(
                    kpg + (int64_t)(jc & page_mask) * kps);
            }
#pragma unroll
            for (int it = 0; it < NLV; ++it) {
                const int j = g0 + 2 * (it * RPL + k_r);
#pragma unroll
                for (int e = 0; e < 2; ++e)
                    vr[it][e] = *reinterpret_cast<const u32x2*>(
                        vpg + (int64_t)(imin(j + e, k_end) & page_mask) * vps);
            }
            if (lane < 32) {
                // the same clamp: no scale of a row beyond k_end is loaded
                const int jc = imin(g0 + lcol, k_end);
                sc = sc_base[scale_row(page) + (jc & page_mask)];
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
        if (g0 + BLOCK_N <= k_end) page = page_of(g0 + BLOCK_N);
    };
    // bytes -> bf16, once per workgroup and GQA group, into the LDS images
    auto store_tile = [&]() {
#pragma unroll
        for (int it = 0; it < NLK; ++it) {
            const int row = wrow + it * RPL + k_r;
            *reinterpret_cast<u32x4*>(&k_lds[row * KSTRIDE + k_col]) =
                fp8x8_to_bf16(kr[it]);
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

    load_tile(k_lo);
    for (int kv0 = k_lo; kv0 <= k_end; kv0 += BLOCK_N) {
        block_barrier();               // every wave is done with the last tile
        store_tile();
        block_barrier();
        if (kv0 + BLOCK_N <= k_end) load_tile(kv0 + BLOCK_N);   // in flight
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
                s_tile[ns][r] = __builtin_fmaf(slope2[r], (float)(jk - prow[r]),
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
                p_lds[(4 * lgrp + r) * VSTRIDE + ns * 16 + lcol] =
                    (__bf16)(pv * vs[ns]);
            }
            ls = group_sum<16>(ls);
            l_run[r] = __builtin_fmaf(l_run[r], rescale, ls);
#pragma unroll
            for (int s = 0; s < DSUB; ++s) accO[s][r] *= rescale;
        }
        wave_sync();                   // own-wave P writes before reads

        // O += (P * vs) V_bytes  (64 keys in 2 chunks of 32)
#pragma unroll
        for (int kc = 0; kc < 2; ++kc) {
            frag_ab aP = *reinterpret_cast<const frag_ab*>(
                &p_lds[lcol * VSTRIDE + kc * 32 + 8 * lgrp]);
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

    // epilogue: real rows only; out-of-range rows are zeros / the empty state
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = wr0 + 4 * lgrp + r;
        const int ti = row >> gshift;
        if (ti >= n_tok) continue;
        const bool live =
            prow[r] >= 0 && prow[r] < capacity && l_run[r] > 0.f;
        if constexpr (SPLIT) {
            if (lcol == 0) {
                part_ml[2 * (wsrow + row)] = live ? m_run[r] : -FLT_MAX;
                part_ml[2 * (wsrow + row) + 1] = live ? l_run[r] : 0.f;
            }
            if (live) {
                float* arow = part_acc + (wsrow + row) * D;
#pragma unroll
                for (int ds = 0; ds < DSUB; ++ds)
                    arow[ds * 16 + lcol] = accO[ds][r];
            }
        } else {
            const float inv_l = live ? 1.0f / l_run[r] : 0.f;
            __bf16* orow = o + (int64_t)imin(tok0 + ti, T - 1) * os
                + (int64_t)(h0 + (row & gmask)) * D;
#pragma unroll
            for (int ds = 0; ds < DSUB; ++ds)
                orow[ds * 16 + lcol] =
                    (__bf16)(live ? accO[ds][r] * inv_l : 0.f);
        }
    }
}

}  // namespace

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

torch::Tensor paged_varlen_split_attn_fp8(
        torch::Tensor q, torch::Tensor k_pool, torch::Tensor v_pool,
        torch::Tensor k_scale, torch::Tensor v_scale,
        torch::Tensor block_table, torch::Tensor slopes, double scale,
        torch::Tensor cu_q, torch::Tensor start, int64_t n_splits,
        bool short_body) {
    const char* op = "paged_varlen_split_attn_fp8";
    TORCH_CHECK(q.dim() == 3 && q.size(0) >= 1, op,
                ": q must be [T, H, D] with T >= 1");
    const int64_t T = q.size(0), H = q.size(1), D = q.size(2);
    check_operand(op, "q", q.unsqueeze(0), {1, T, H, D});
    TORCH_CHECK(cu_q.is_cuda() && cu_q.scalar_type() == torch::kInt &&
                cu_q.dim() == 1 && cu_q.is_contiguous() && cu_q.numel() >= 2,
                op, ": cu_q must be a contiguous int32 GPU tensor of B + 1 "
                "elements");
    const int64_t B = cu_q.numel() - 1;
    TORCH_CHECK(B <= MAX_SEQS, op, ": at most ", MAX_SEQS,
                " sequences per call, got ", B);
    TORCH_CHECK(T <= MAX_TOKENS, op, ": at most ", MAX_TOKENS,
                " packed rows per call, got ", T);
    const int shift = check_paged_fp8(op, k_pool, v_pool, k_scale, v_scale,
                                      block_table, B, D, q.device());
    const int64_t n_pages = k_pool.size(0), Hkv = k_pool.size(1);
    const int64_t capacity = block_table.size(1) << shift;
    TORCH_CHECK(H > 0 && H % Hkv == 0, op,
                ": q heads must be a multiple of kv heads");
    TORCH_CHECK(slopes.is_cuda() && slopes.scalar_type() == torch::kFloat &&
                slopes.numel() == H && slopes.is_contiguous(), op,
                ": slopes must be ", H, " contiguous fp32 values on the GPU");
    check_position(op, "start", start, B);
    TORCH_CHECK(cu_q.device() == q.device() && start.device() == q.device() &&
                slopes.device() == q.device(), op,
                ": all operands must be on the same device");

    const decode_common::SplitPlan plan = decode_common::make_split_plan(
        op, T, B, H, Hkv, capacity, n_splits);
    TORCH_CHECK(plan.ny <= 65535, op, ": H must fit a grid dimension");
    const int64_t ws_rows = plan.n_slot * plan.n_splits * plan.ny * BLOCK_M;
    TORCH_CHECK(plan.n_splits == 1 ||
                ws_rows * (D + 2) * 4 <= decode_common::MAX_WORKSPACE,
                op, ": n_splits = ", plan.n_splits, " needs a workspace of ",
                ws_rows * (D + 2) * 4, " bytes, more than ",
                decode_common::MAX_WORKSPACE, "; use fewer splits");

    auto o = torch::empty({T, H, D}, q.options());
    torch::Tensor part_acc, part_ml;
    float *acc_p = nullptr, *ml_p = nullptr;
    if (plan.n_splits > 1) {
        const auto f32 = q.options().dtype(torch::kFloat);
        part_acc = torch::empty({ws_rows, D}, f32);
        part_ml = torch::empty({ws_rows, 2}, f32);
        acc_p = part_acc.data_ptr<float>();
        ml_p = part_ml.data_ptr<float>();
    }
    auto stream = at::cuda::getCurrentCUDAStream();
    const dim3 grid((unsigned)plan.n_slot, (unsigned)plan.ny,
                    (unsigned)plan.n_splits);
    auto launch = [&](auto dv_, auto split_) {
        constexpr int DV = decltype(dv_)::value;
        constexpr bool SP = decltype(split_)::value;
        hipLaunchKernelGGL((paged_varlen_split_attn_fp8_kernel<DV, SP>), grid,
                           dim3(NW * WAVE_SIZE), 0, stream,
                           reinterpret_cast<const __bf16*>(q.data_ptr()),
                           reinterpret_cast<const uint8_t*>(k_pool.data_ptr()),
                           reinterpret_cast<const uint8_t*>(v_pool.data_ptr()),
                           k_scale.data_ptr<float>(),
                           v_scale.data_ptr<float>(),
                           block_table.data_ptr<int>(), block_table.stride(0),
                           slopes.data_ptr<float>(), (float)scale,
                           cu_q.data_ptr<int>(),
                           start.data_ptr<int64_t>(), (int)start.numel(),
                           reinterpret_cast<__bf16*>(o.data_ptr()), acc_p, ml_p,
                           (int)T, (int)B, (int)H, (int)(H / Hkv), plan.gshift,
                           (int)short_body, (int)plan.n_slot, (int)plan.ny,
                           plan.n_splits,
                           (int)capacity, (int)n_pages, shift,
                           q.stride(0), q.stride(1),
                           k_pool.stride(0), k_pool.stride(1), k_pool.stride(2),
                           v_pool.stride(0), v_pool.stride(1),
                           v_pool.stride(2));
        if constexpr (SP)
            decode_common::launch_split_combine(
                acc_p, ml_p, cu_q.data_ptr<int>(),
                reinterpret_cast<__hip_bfloat16*>(o.data_ptr()), plan, T, B,
                H, D);
    };
    using std::integral_constant;
    if (D == 64 && plan.n_splits == 1)
        launch(integral_constant<int, 64>{}, std::false_type{});
    else if (D == 64)
        launch(integral_constant<int, 64>{}, std::true_type{});
    else if (plan.n_splits == 1)
        launch(integral_constant<int, 128>{}, std::false_type{});
    else
        launch(integral_constant<int, 128>{}, std::true_type{});
    HIP_CHECK_LAUNCH();
    return o;
}
