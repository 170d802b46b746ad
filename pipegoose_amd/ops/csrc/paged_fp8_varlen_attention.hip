// Ragged-batch paged attention over the fp8 cache for gfx950: the semantics
// of paged_varlen_attn (header of paged_varlen_attention.hip) over the
// storage of paged_fp8_attention.hip.
//
//   q [T,H,D] bf16, token-packed; cu_q int32 [B+1] and start int64 [B] (or one
//   element for all), both READ ON THE DEVICE; row t of sequence b sits at
//   p = start[b] + (t - cu_q[b]) and sees keys 0..p through block_table[b]
//
//   k_pool, v_pool   [n_pages, Hkv, PAGE, D]  OCP e4m3fn, one byte per element
//   k_scale, v_scale [n_pages, Hkv, PAGE]     fp32, contiguous, same page ids
//   a value reads back as float(byte) * scale
//
//   o[t,h,:] = softmax_j( scale * q[t,h,:]·K[b,h/G,j,:] + slopes[h]*(j - p) )
//              @ V[b,h/G,j,:]           j in [0, p]
//
// o is [T,H,D], bf16, contiguous.  Rows t >= cu_q[B] are padding and give
// exact zeros, rows with p outside [0, max_pages*PAGE) give exact zeros, a
// sequence may own zero rows, B <= 1024 and T <= 2^20.
//
// Work split: the varlen kernel's.  A workgroup is 4 waves x 16 rows of a
// 64-row M tile, v_mfma_f32_16x16x32_bf16, and the 64 rows are TPT = 64/gp
// tokens x gp heads of ONE kv head (gp = G when G is in {1,2,4,8,16}, else
// 1): tile row r is token r >> log2(gp) and head h0 + (r & (gp-1)).  The grid
// is (ceil(T/TPT) + B, H/gp), from shapes only (graph-capturable); each
// workgroup finds its (sequence, tile) by a wave scan of the clamped cu_q, 64
// sequences a step, and the workgroups past the last tile zero the padding
// rows.  Position, causal cut and slope are per-row quantities, 4 per lane in
// the C layout.  A tile with no in-range row writes zeros and loads nothing.
//
// Data movement: the fp8 prefill kernel's.  A wave stages rows [16w, 16w+16)
// of each 64-key tile: one page (PAGE >= 16), one wave-uniform table read,
// fetched a tile ahead.  The prefetch registers hold BYTES in 8-byte packets,
// half of the bf16 kernel's kr/vr, and the 16 K scales and 16 V scales of
// those rows ride with them in lanes 0..15 and 16..31.  store_tile converts
// once per workgroup (v_cvt_pk_f32_fp8, the upper halves of the fp32, which
// is exact, packed by v_perm_b32) into the bf16 LDS images, K row-major on
// padded rows and V transposed, and puts the scales into ks_lds[64] /
// vs_lds[64].  Here that one conversion serves the whole GQA group: the
// prefill kernel converts a tile once per head, this one once per kv head.
//
// Scales.  The K scale enters the score as acc * (scale2 * ks), the V scale
// multiplies the softmax weight before its bf16 rounding into p_lds, l sums
// the UNSCALED fp32 weights.  No dequantised element is scaled on its own.
//
// What is never read: both parents' rules, for bytes AND scales.  p_max is
// the largest in-range position of the workgroup's real rows; the key loop
// runs p_max/64 + 1 tiles; row indices are clamped to p_max; a wave whose 16
// staged rows start beyond p_max loads nothing and stages zero bytes and
// scale 0; table entries with index > p_max / PAGE are never read; every page
// id is clamped into [0, n_pages-1]; every value read from cu_q is clamped
// into [0, T], so a corrupt cu_q gives wrong numbers (rows left unwritten
// included), never an out-of-bounds access.  A masked column holds the bytes
// and scale of row p_max, or zeros and scale 0, never a tail value: masking
// is a select on the score and on the weight, and 0 * scale is finite.
//
// No atomics, no split-KV: results are bit-reproducible for fixed inputs.
//
// The cu_q scan and the padding zeroing repeat those of
// paged_varlen_attention.hip instead of sharing a header with it: that file
// writes them with the HIP headers' shuffles and ballot, which cannot inline
// into device code built with packed-fp32-ops off (below), so a shared
// version would have to rewrite the bf16 kernel's scan on raw builtins, and
// its recorded resource numbers were not worth putting at stake for 40 lines.
//
// Resources (hipcc -O3 --offload-arch=gfx950
// -Rpass-analysis=kernel-resource-usage):
//   D = 64 : 120 VGPRs + 16 AGPRs, 84 SGPRs, 28160 B LDS, 3 waves/SIMD
//   D = 128: 154 VGPRs + 32 AGPRs, 84 SGPRs, 45568 B LDS, 2 waves/SIMD
// no scratch at either head dim.  The waves/SIMD are those of the bf16 varlen
// kernel (133 / 175 VGPRs, 27648 / 45056 B LDS): the byte prefetch saves more
// registers than the scales cost, and the 512 B of scale LDS cost no wave.
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

#include <cfloat>
#include <type_traits>

#include "attn_checks.h"
#include "common.h"

// Compiled with the packed-fp32-ops target feature off, for the reason in
// the header of paged_fp8_attention.hip; as there, device code below calls
// compiler builtins only (profiles/paged_fp8_varlen_attn.md).
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
constexpr int BLOCK_N = 64;   // keys per LDS tile
constexpr int NW = 4;         // waves per workgroup, 16 rows each
constexpr int PAD = 8;        // bf16 elements (16 B) of row padding in LDS
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

// x of lane `src` of the wave (ds_bpermute); every lane is active wherever
// this is used, and a src below 0 is never consumed
__device__ __forceinline__ int lane_read(int x, int src) {
    return __builtin_amdgcn_ds_bpermute(src << 2, x);
}

// Pool strides are in bytes (= elements).  Hkv = H / G.
template <int D>
__global__ __launch_bounds__(NW * WAVE_SIZE)
void paged_varlen_attn_fp8_kernel(const __bf16* __restrict__ q,
                                  const uint8_t* __restrict__ k_pool,
                                  const uint8_t* __restrict__ v_pool,
                                  const float* __restrict__ k_scale,
                                  const float* __restrict__ v_scale,
                                  const int* __restrict__ block_table,
                                  int64_t bt_stride,
                                  const float* __restrict__ slopes,
                                  float scale,
                                  const int* __restrict__ cu_q,
                                  const int64_t* __restrict__ start,
                                  int start_n,
                                  __bf16* __restrict__ o,       // [T,H,D]
                                  int T, int B, int H, int G, int gshift,
                                  int n_wg, int capacity, int n_pages,
                                  int page_shift,
                                  int64_t qt, int64_t qh,
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

    const int wg = __builtin_amdgcn_workgroup_id_x();
    const int tid = __builtin_amdgcn_workitem_id_x();
    const int wave = tid / WAVE_SIZE;
    const int lane = tid % WAVE_SIZE;
    const int lgrp = lane >> 4;       // 0..3
    const int lcol = lane & 15;       // 0..15
    const int gmask = (1 << gshift) - 1;
    const int tpt_shift = 6 - gshift;           // TPT = 64 >> gshift tokens
    const int TPT = 1 << tpt_shift;
    const int h0 = __builtin_amdgcn_workgroup_id_y() << gshift;
    const int hk = h0 / G;
    const int Hkv = H / G;
    const int64_t os = (int64_t)H * D;

    auto cu = [&](int i) { return imin(imax(cu_q[i], 0), T); };

    // ---- which (sequence, tile) is this workgroup?  Every wave scans alone:
    // the results are wave-uniform and equal in all four
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
        // past the last tile: the zeros of the padding rows, strided over
        // the surplus workgroups; each thread one 16-byte packet at a time
        const int n_surplus = n_wg - total;     // n_wg = the grid's x extent
        const int row = tid >> 2;               // tile row 0..63
        const int head = h0 + (row & gmask);
        for (int64_t t = (int64_t)cu(B) + (int64_t)(wg - total) * TPT
                 + (row >> gshift);
             t < T; t += (int64_t)n_surplus * TPT) {
            __bf16* orow = o + t * os + (int64_t)head * D;
            for (int c = (tid & 3) * 8; c < D; c += 32)
                *reinterpret_cast<u32x4*>(orow + c) = u32x4{0u, 0u, 0u, 0u};
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
    const int wr0 = wave * 16;                  // this wave's first tile row

    if (p_lo > p_max) {
        // no row of the tile is in range: zeros, and nothing is loaded
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = wr0 + 4 * lgrp + r;
            const int ti = row >> gshift;
            if (ti < n_tok) {
                __bf16* orow = o + (int64_t)imin(tok0 + ti, T - 1) * os
                    + (int64_t)(h0 + (row & gmask)) * D;
#pragma unroll
                for (int ds = 0; ds < DSUB; ++ds)
                    orow[ds * 16 + lcol] = (__bf16)0.f;
            }
        }
        return;
    }

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
    const float scale2 = scale * LOG2E;              // exp2 domain

    int prow[4];                                     // position of C-row r
    float slope2[4];                                 // its head's slope
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = wr0 + 4 * lgrp + r;
        prow[r] = st + i0 + (row >> gshift);
        slope2[r] = slopes[h0 + (row & gmask)] * LOG2E;
    }

    frag_cd accO[DSUB];
    float m_run[4], l_run[4];
#pragma unroll
    for (int s = 0; s < DSUB; ++s) accO[s] = frag_cd{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int r = 0; r < 4; ++r) { m_run[r] = -FLT_MAX; l_run[r] = 0.f; }

    // ---- staging: this wave moves rows [16*wave, 16*wave+16) of each tile
    const int* bt_row = block_table + seq * bt_stride;
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
    // bytes -> bf16, once per workgroup and GQA group, into the LDS images
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
        const int row = wr0 + 4 * lgrp + r;
        const int ti = row >> gshift;
        if (ti >= n_tok) continue;
        const bool in_range = prow[r] >= 0 && prow[r] < capacity;
        const float inv_l = in_range ? 1.0f / l_run[r] : 0.f;
        __bf16* orow = o + (int64_t)imin(tok0 + ti, T - 1) * os
            + (int64_t)(h0 + (row & gmask)) * D;
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

torch::Tensor paged_varlen_attn_fp8(torch::Tensor q, torch::Tensor k_pool,
                                    torch::Tensor v_pool,
                                    torch::Tensor k_scale,
                                    torch::Tensor v_scale,
                                    torch::Tensor block_table,
                                    torch::Tensor slopes, double scale,
                                    torch::Tensor cu_q, torch::Tensor start) {
    const char* op = "paged_varlen_attn_fp8";
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

    // the GQA group shares a tile when it divides the 64 rows
    const int64_t G = H / Hkv;
    int gshift = 0;
    if (G == 2 || G == 4 || G == 8 || G == 16)
        while ((1 << gshift) < G) ++gshift;
    const int64_t gp = (int64_t)1 << gshift, tpt = BLOCK_M / gp;
    TORCH_CHECK(H / gp <= 65535, op, ": H must fit a grid dimension");

    auto o = torch::empty({T, H, D}, q.options());
    auto stream = at::cuda::getCurrentCUDAStream();
    const int64_t n_wg = (T + tpt - 1) / tpt + B;
    auto launch = [&](auto dv_) {
        constexpr int DV = decltype(dv_)::value;
        hipLaunchKernelGGL((paged_varlen_attn_fp8_kernel<DV>),
                           dim3((unsigned)n_wg, (unsigned)(H / gp)),
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
                           reinterpret_cast<__bf16*>(o.data_ptr()),
                           (int)T, (int)B, (int)H, (int)G, gshift,
                           (int)n_wg, (int)capacity, (int)n_pages, shift,
                           q.stride(0), q.stride(1),
                           k_pool.stride(0), k_pool.stride(1), k_pool.stride(2),
                           v_pool.stride(0), v_pool.stride(1),
                           v_pool.stride(2));
    };
    if (D == 64) launch(std::integral_constant<int, 64>{});
    else launch(std::integral_constant<int, 128>{});
    HIP_CHECK_LAUNCH();
    return o;
}
