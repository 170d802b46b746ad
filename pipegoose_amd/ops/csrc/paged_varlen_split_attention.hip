// Split-KV ragged-batch paged attention for gfx950: paged_varlen_attn
// (paged_varlen_attention.hip) with the keys of every M tile divided among
// n_splits workgroups, and a body for tiles that hold decode rows.  Operands,
// semantics and the "what is never read" rules are those of that file's
// header and all carry over: q [T,H,D] bf16, bf16 pools, block_table
// [B,max_pages], slopes; cu_q int32 [B+1] and start int64 READ ON THE DEVICE;
// padding rows and rows outside [0, max_pages*PAGE) give exact zeros; every
// id and every cu_q value clamped; nothing past the largest visible position
// loaded, table entries included.  One more argument, n_splits (0 = auto,
// 1..MAX_SPLITS forced); o [T,H,D] bf16.  No atomics: results are
// bit-reproducible for fixed inputs and plan.
//
// Work split.  The M tile is the sibling's: 64 rows = 64/gp tokens x the gp
// heads of one kv head, a tile never crosses a sequence, grid x = N_slot =
// ceil(T/TPT) + B tile slots found by the in-kernel cu_q scan (find_tile,
// used by both kernels here), grid y = H/gp.  Grid z = n_splits.
//
// Host plan (shapes only, so a captured call replays with cu_q / start /
// table as data): n_splits = clamp(ceil(TARGET_WGS / (N_slot*H/gp)), 1,
// min(MAX_SPLITS, capacity/64)), constants from decode_common.h.  A large
// packed prefill gets 1, and with n_splits == 1 the kernel writes o itself:
// no workspace, no combine launch.
//
// Device plan, per tile.  n_keys = p_max + 1 (p_max: the largest in-range
// position of the tile's real rows), chunk = round_up(ceil(n_keys /
// n_splits), 64), split s owns keys [s*chunk, min((s+1)*chunk, n_keys)): a
// long context uses all its splits whatever the capacity.  A split with
// s*chunk > p_max is dead: it writes the empty state (m = -FLT_MAX, l = 0)
// for the tile's real rows and returns without touching K, V or the table.
// In a live split a row with prow < s*chunk sees no key; every score and
// weight is a select on the causal test, so such a row keeps m = -FLT_MAX,
// l = 0, acc = 0 and never evaluates exp2(x - x) of masked scores.  The
// chunk is a multiple of the key tile, so the last key of a split is either
// the last key of a key tile or p_max, and keys past it inside the tile are
// masked by the causal test alone.
//
// Partials: fp32 (m, l) and acc[D], unnormalised, exp2 domain, in a workspace
// indexed (slot, split, y, tile row) that the op allocates with torch::empty.
// Only real rows are written, acc only for in-range rows.
//
// Combine kernel (paged_varlen_split_combine_kernel): one workgroup per
// (slot, y); repeats the scan, merges the splits in split order, SELECTS on
// l == 0 (the workspace is uninitialised and 0 * NaN is NaN: an empty
// split's acc is never read), writes bf16 o for real rows, zeros for rows
// all of whose splits are empty (the out-of-range rows), and the padding
// zeros from the surplus slots.
//
// Bodies.  The shared-tile body is the sibling's key loop (64-key tiles staged
// through LDS by all four waves, P bounced through LDS, one tile prefetched
// in registers) run over the split's keys.  A tile is SHORT when n_tok * gp
// <= 16 (workgroup-uniform): all its real rows sit in wave 0's 16 rows, the
// other three waves would stage and idle, and every key tile would cost two
// workgroup barriers.  In the short body each of the 4 waves serves the same
// 16 rows against its own 16-key slice of every 64-key tile (16-aligned,
// inside one page for every allowed PAGE, one wave-uniform table lookup):
//   - K goes from HBM straight into the MFMA B operand (lane = key row lcol,
//     8 contiguous bf16 at c*32 + 8*lgrp); it never passes through LDS, each
//     element is used once;
//   - V^T and P go through the wave's private LDS slice; the key loop has
//     wave-level synchronisation only, no __syncthreads;
//   - PV is a 16x16x32 MFMA whose upper 16 k-lanes (lgrp 2, 3) carry zeros
//     in both operands: the matrix pipe is idle in this body anyway;
//   - each wave keeps its own (m, l, accO); the four states merge once at
//     the end through LDS, in wave order, and all 256 threads write the
//     result: the partial, or o when n_splits == 1.
// short_body = false (binding argument, for measurements) runs every tile
// through the shared-tile body.  The short body is kept: on decode-only rows
// it takes 0.77-1.00x the shared-tile body's time from context 1024 up and
// ties within the spread below (profiles/paged_mixed_attn.md has both).
//
// Resources (hipcc -O3 --offload-arch=gfx950
// -Rpass-analysis=kernel-resource-usage), n_splits == 1 / n_splits > 1:
//   D = 64 : 138 / 135 VGPRs + 16 AGPRs, 83 / 75 SGPRs, 27648 B LDS,
//            3 waves/SIMD
//   D = 128: 181 / 177 VGPRs + 32 AGPRs, 83 / 75 SGPRs, 45056 B LDS,
//            2 waves/SIMD
//   combine: 46 (D = 64) / 79 (D = 128) VGPRs, no LDS, 8 / 6 waves/SIMD
// no scratch in any of them: the waves/SIMD of paged_varlen_attn.
//
// The host plan (make_split_plan) and the launcher of the combine kernel
// (launch_split_combine) are declared in decode_common.h and defined below:
// paged_fp8_varlen_split_attention.hip uses both, so the fp8 kernel has this
// plan and this combine kernel, not copies.
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

#include <cfloat>
#include <tuple>
#include <type_traits>

#include "attn_checks.h"
#include "decode_common.h"
#include "mfma_frag.h"

namespace {

constexpr int BLOCK_M = 64;   // (token, head) rows per workgroup
constexpr int BLOCK_N = 64;   // keys per key tile
constexpr int NW = 4;         // waves per workgroup
constexpr int PAD = 8;        // bf16 elements (16 B) of row padding in LDS
constexpr int SV = 16 + PAD;  // row stride of a wave's private 16-key slices
constexpr int MAX_SEQS = 1024;
constexpr int MAX_TOKENS = 1 << 20;
using decode_common::MAX_WORKSPACE;
using decode_common::SplitPlan;
constexpr float LOG2E = 1.4426950408889634f;

struct TileId {
    int seq, tile, total;   // seq < 0: a surplus slot, total tiles in all
};

__device__ __forceinline__ int cu_at(const int* __restrict__ cu_q, int i,
                                     int T) {
    return min(max(cu_q[i], 0), T);
}

// Which (sequence, tile within it) is slot wg?  The scan of
// paged_varlen_attention.hip: every wave alone, 64 sequences at a time
// (shuffle prefix sum of the tile counts, ballot for the first sequence
// whose running total passes wg); the result is wave-uniform.
__device__ __forceinline__ TileId find_tile(const int* __restrict__ cu_q,
                                            int B, int T, int tpt_shift,
                                            int wg, int lane) {
    const int TPT = 1 << tpt_shift;
    int total = 0, seq = -1, tile = 0;
    for (int base = 0; base < B; base += WAVE_SIZE) {
        const int b = base + lane;
        int n = 0;
        if (b < B)
            n = (max(cu_at(cu_q, b + 1, T) - cu_at(cu_q, b, T), 0) + TPT - 1)
                >> tpt_shift;
        int incl = n;
#pragma unroll
        for (int off = 1; off < WAVE_SIZE; off <<= 1) {
            const int up = __shfl_up(incl, off, WAVE_SIZE);
            if (lane >= off) incl += up;
        }
        incl += total;
        const unsigned long long hit = __ballot(incl > wg);
        if (seq < 0 && hit != 0) {              // wave-uniform
            const int l = __ffsll((long long)hit) - 1;
            seq = base + l;
            tile = wg - __shfl(incl - n, l, WAVE_SIZE);
        }
        total = __shfl(incl, WAVE_SIZE - 1, WAVE_SIZE);
    }
    return {__builtin_amdgcn_readfirstlane(seq),
            __builtin_amdgcn_readfirstlane(tile),
            __builtin_amdgcn_readfirstlane(total)};
}

// The zeros of the padding rows t >= cu_q[B], strided over the surplus
// slots; each thread one 16-byte packet at a time.
template <int D>
__device__ __forceinline__ void write_padding(bf16* __restrict__ o, int first,
                                              int surplus, int n_surplus,
                                              int T, int H, int h0,
                                              int gshift, int tid) {
    const int TPT = BLOCK_M >> gshift;
    const int row = tid >> 2;               // tile row 0..63
    const int head = h0 + (row & ((1 << gshift) - 1));
    for (int64_t t = (int64_t)first + (int64_t)surplus * TPT + (row >> gshift);
         t < T; t += (int64_t)n_surplus * TPT) {
        bf16* orow = o + (t * H + head) * D;
        for (int c = (tid & 3) * 8; c < D; c += 32)
            *reinterpret_cast<frag_ab*>(orow + c) = frag_ab{};
    }
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
    static constexpr int SHARED =
        (BLOCK_N * KSTRIDE + D * VSTRIDE + NW * 16 * VSTRIDE) * 2;
    static constexpr int SLICE = (D + 16) * SV;            // bf16 per wave
    static constexpr int MSTRIDE = D + 2;                  // acc, m, l
    static constexpr int MERGE = NW * 16 * MSTRIDE * 4;
    static_assert(NW * SLICE * 2 <= SHARED && MERGE <= SHARED, "LDS reuse");
};

template <int D, bool SPLIT>
__global__ __launch_bounds__(NW * WAVE_SIZE)
void paged_varlen_split_attn_kernel(
        const bf16* __restrict__ q, const bf16* __restrict__ k_pool,
        const bf16* __restrict__ v_pool, const int* __restrict__ block_table,
        int64_t bt_stride, const float* __restrict__ slopes, float scale,
        const int* __restrict__ cu_q, const int64_t* __restrict__ start,
        int start_n,
        bf16* __restrict__ o,                 // [T,H,D]
        float* __restrict__ part_acc,         // [slot,split,y,64,D]
        float* __restrict__ part_ml,          // [slot,split,y,64,2]
        int T, int B, int H, int G, int gshift, int short_body,
        int capacity, int n_pages, int page_shift,
        int64_t qt, int64_t qh,
        int64_t kpp, int64_t kph, int64_t kps,
        int64_t vpp, int64_t vph, int64_t vps) {
    constexpr int DCH = D / 32;     // K-chunks per QK^T mfma row
    constexpr int DSUB = D / 16;    // output d-subtiles
    constexpr int KSTRIDE = Lds<D>::KSTRIDE;
    constexpr int VSTRIDE = Lds<D>::VSTRIDE;
    constexpr int MSTRIDE = Lds<D>::MSTRIDE;
    constexpr int TPR = D / 8;      // 16-byte packets per row
    constexpr int RPI = WAVE_SIZE / TPR;        // rows per load iteration
    constexpr int NLK = 16 / RPI;               // K loads per lane and tile
    constexpr int NLV = 8 / RPI;                // V row-pair loads per lane

    __shared__ __attribute__((aligned(16))) char lds_raw[Lds<D>::SHARED];

    const int wg = blockIdx.x;
    const int tid = threadIdx.x;
    const int wave = tid / WAVE_SIZE;
    const int lane = tid % WAVE_SIZE;
    const int lgrp = lane >> 4;       // 0..3
    const int lcol = lane & 15;       // 0..15
    const int gmask = (1 << gshift) - 1;
    const int tpt_shift = 6 - gshift;           // TPT = 64 >> gshift tokens
    const int TPT = 1 << tpt_shift;
    const int h0 = blockIdx.y << gshift;        // first head of the tile
    const int hk = h0 / G;
    const int64_t os = (int64_t)H * D;

    const TileId id = find_tile(cu_q, B, T, tpt_shift, wg, lane);
    if (id.seq < 0) {
        if constexpr (!SPLIT)
            write_padding<D>(o, cu_at(cu_q, B, T), wg - id.total,
                             (int)gridDim.x - id.total, T, H, h0, gshift, tid);
        return;                     // SPLIT: the combine kernel writes them
    }
    const int seq = id.seq;
    const int c0 = cu_at(cu_q, seq, T);
    const int len = max(cu_at(cu_q, seq + 1, T) - c0, 0);
    const int i0 = id.tile << tpt_shift;        // first row of the tile in seq
    const int n_tok = min(TPT, len - i0);       // real tokens here, >= 1
    const int tok0 = c0 + i0;                   // packed index, tok0+n_tok <= T

    // capacity and T are < 2^30: a start below -2^30 or at or above capacity
    // puts every row out of range either way, and clamped to that interval
    // all the int arithmetic below is exact
    int64_t st64 = start[start_n == 1 ? 0 : seq];
    st64 = st64 < -((int64_t)1 << 30) ? -((int64_t)1 << 30) : st64;
    const int st = (int)(st64 > capacity ? capacity : st64);

    const int p_lo = max(st + i0, 0);
    const int p_max = min(st + i0 + n_tok - 1, capacity - 1);

    // this workgroup's rows of the partial workspace
    const int split = blockIdx.z, nsp = gridDim.z;
    const int64_t wsrow =
        (((int64_t)wg * nsp + split) * gridDim.y + blockIdx.y) * BLOCK_M;

    // the device plan: keys [k_lo, k_end] of this split (file header)
    int k_lo = 0, k_end = p_max;
    bool dead = p_lo > p_max;       // no row of the tile is in range
    if (SPLIT && !dead) {
        const int chunk =
            ((p_max + nsp) / nsp + BLOCK_N - 1) & ~(BLOCK_N - 1);
        k_lo = split * chunk;       // < n_keys + 65 * nsp: no overflow
        k_end = min(k_lo + chunk, p_max + 1) - 1;
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
                bf16* orow = o + (int64_t)min(tok0 + ti, T - 1) * os
                    + (int64_t)(h0 + (row & gmask)) * D;
                for (int c = (tid & 3) * 8; c < D; c += 32)
                    *reinterpret_cast<frag_ab*>(orow + c) = frag_ab{};
            }
        }
        return;
    }

    const float scale2 = scale * LOG2E;              // exp2 domain
    const int* bt_row = block_table + seq * bt_stride;
    const int page_mask = (1 << page_shift) - 1;
    auto page_of = [&](int row) {
        const int id = bt_row[__builtin_amdgcn_readfirstlane(row) >> page_shift];
        return min(max(id, 0), n_pages - 1);
    };
    const bf16* kbase = k_pool + hk * kph;
    const bf16* vbase = v_pool + hk * vph;
    const int wrow = __builtin_amdgcn_readfirstlane(wave * 16);
    const int k_r = lane / TPR, k_col = (lane % TPR) * 8;   // + it*RPI rows

    frag_cd accO[DSUB];
    float m_run[4], l_run[4];
#pragma unroll
    for (int s = 0; s < DSUB; ++s) accO[s] = frag_cd{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int r = 0; r < 4; ++r) { m_run[r] = -FLT_MAX; l_run[r] = 0.f; }

    if (short_body && (n_tok << gshift) <= 16) {
        // ================= short tile: 4 waves x 16 keys, the same 16 rows
        bf16* vts = reinterpret_cast<bf16*>(lds_raw) + wave * Lds<D>::SLICE;
        bf16* ps = vts + D * SV;

        frag_ab aQ[DCH];
        {
            const int tg =
                min(max(tok0 + min(lcol >> gshift, n_tok - 1), 0), T - 1);
            const bf16* qrow = q + tg * qt + (int64_t)(h0 + (lcol & gmask)) * qh;
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

        // the wave's 16 keys of the tile at kv0, K in B-operand layout; a
        // slice that starts past k_end is not loaded (and ends the loop)
        frag_ab kn[DCH], vn[NLV][2];
        auto load_slice = [&](int kv0) {
            const int g0 = kv0 + wrow;
            if (g0 > k_end) return;                     // wave-uniform
            const int page = page_of(g0);
            const bf16* kpg = kbase + page * kpp
                + (int64_t)(min(g0 + lcol, k_end) & page_mask) * kps + 8 * lgrp;
#pragma unroll
            for (int c = 0; c < DCH; ++c)
                kn[c] = *reinterpret_cast<const frag_ab*>(kpg + c * 32);
            const bf16* vpg = vbase + page * vpp + k_col;
#pragma unroll
            for (int it = 0; it < NLV; ++it) {
                const int j = g0 + 2 * (it * RPI + k_r);
#pragma unroll
                for (int e = 0; e < 2; ++e)
                    vn[it][e] = *reinterpret_cast<const frag_ab*>(
                        vpg + (int64_t)(min(j + e, k_end) & page_mask) * vps);
            }
        };

        load_slice(k_lo);
        for (int kv0 = k_lo; kv0 + wrow <= k_end; kv0 += BLOCK_N) {
            frag_ab kc[DCH];
#pragma unroll
            for (int c = 0; c < DCH; ++c) kc[c] = kn[c];
#pragma unroll
            for (int it = 0; it < NLV; ++it) {
                // V transposed; two rows at once -> 4-byte column stores
                const int row = 2 * (it * RPI + k_r);
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    union { __bf16 h[2]; uint32_t u; } pair;
                    pair.h[0] = vn[it][0][j];
                    pair.h[1] = vn[it][1][j];
                    *reinterpret_cast<uint32_t*>(
                        &vts[(k_col + j) * SV + row]) = pair.u;
                }
            }
            load_slice(kv0 + BLOCK_N);                  // in flight below

            frag_cd acc = frag_cd{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int c = 0; c < DCH; ++c) acc = MFMA_16x16x32(aQ[c], kc[c], acc);
            const int jk = kv0 + wrow + lcol;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const bool ok = jk <= prow[r];
                const float s = fmaf(slope2[r], (float)(jk - prow[r]),
                                     acc[r] * scale2);
                float mx = ok ? s : -FLT_MAX;
#pragma unroll
                for (int off = 1; off < 16; off <<= 1)
                    mx = fmaxf(mx, __shfl_xor(mx, off, WAVE_SIZE));
                const float m_new = fmaxf(m_run[r], mx);
                const float rescale = __builtin_amdgcn_exp2f(m_run[r] - m_new);
                m_run[r] = m_new;
                const float pv = ok ? __builtin_amdgcn_exp2f(s - m_new) : 0.f;
                ps[(4 * lgrp + r) * SV + lcol] = (bf16)pv;
                float ls = pv;
#pragma unroll
                for (int off = 1; off < 16; off <<= 1)
                    ls += __shfl_xor(ls, off, WAVE_SIZE);
                l_run[r] = fmaf(l_run[r], rescale, ls);
#pragma unroll
                for (int s2 = 0; s2 < DSUB; ++s2) accO[s2][r] *= rescale;
            }
            wave_sync();            // own-wave V^T and P writes before reads

            // O += P V: k-lanes 0..15 are the keys, 16..31 zeros
            frag_ab aP = frag_ab{};
            if (lgrp < 2)
                aP = *reinterpret_cast<const frag_ab*>(&ps[lcol * SV + 8 * lgrp]);
#pragma unroll
            for (int ds = 0; ds < DSUB; ++ds) {
                frag_ab bV = frag_ab{};
                if (lgrp < 2)
                    bV = *reinterpret_cast<const frag_ab*>(
                        &vts[(ds * 16 + lcol) * SV + 8 * lgrp]);
                accO[ds] = MFMA_16x16x32(aP, bV, accO[ds]);
            }
            wave_sync();            // reads before the next slice's writes
        }

        // the four waves' states -> LDS -> merged in wave order by all
        float* sm = reinterpret_cast<float*>(lds_raw);
        __syncthreads();            // every wave has left its slices
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float* srow = sm + (wave * 16 + 4 * lgrp + r) * MSTRIDE;
#pragma unroll
            for (int ds = 0; ds < DSUB; ++ds) srow[ds * 16 + lcol] = accO[ds][r];
            if (lcol == 0) { srow[D] = m_run[r]; srow[D + 1] = l_run[r]; }
        }
        __syncthreads();
        const int row = tid >> 4, cl = tid & 15;    // 16 rows x 16 columns
        float m = -FLT_MAX, l = 0.f, a[DSUB];
#pragma unroll
        for (int ds = 0; ds < DSUB; ++ds) a[ds] = 0.f;
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            const float* srow = sm + (w * 16 + row) * MSTRIDE;
            const float m2 = srow[D], l2 = srow[D + 1];
            if (l2 > 0.f) {
                const float mn = fmaxf(m, m2);
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
            bf16* orow = o + (int64_t)min(tok0 + ti, T - 1) * os
                + (int64_t)(h0 + (row & gmask)) * D;
#pragma unroll
            for (int ds = 0; ds < DSUB; ++ds)
                orow[ds * 16 + cl] = (bf16)(live ? a[ds] * inv_l : 0.f);
        }
        return;
    }

    // ===================== shared tile: the sibling's loop over [k_lo, k_end]
    bf16* k_lds = reinterpret_cast<bf16*>(lds_raw);
    bf16* vt_lds = k_lds + BLOCK_N * KSTRIDE;
    bf16* p_lds = vt_lds + D * VSTRIDE + wave * 16 * VSTRIDE;
    const int wr0 = wave * 16;                  // this wave's first tile row

    // the largest in-range position of this wave's real rows (-1: none):
    // key tiles that start beyond it are wholly masked for the wave
    const int wt0 = wr0 >> gshift, wt1 = (wr0 + 15) >> gshift;
    const int pw_max =
        wt0 < n_tok ? min(st + i0 + min(wt1, n_tok - 1), capacity - 1) : -1;

    frag_ab aQ[DCH];
    {
        // A-fragment row = lcol; rows past the last real token re-read it
        const int row = wr0 + lcol;
        const int tg = min(max(tok0 + min(row >> gshift, n_tok - 1), 0), T - 1);
        const bf16* qrow = q + tg * qt + (int64_t)(h0 + (row & gmask)) * qh;
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

    // ---- staging: this wave moves rows [16*wave, 16*wave+16) of each tile
    frag_ab kr[NLK], vr[NLV][2];
    int page = 0;
    if (k_lo + wrow <= k_end) page = page_of(k_lo + wrow);

    // fetch the wave's part of the tile at kv0 into registers, then the page
    // id of the NEXT tile if the wave will load there
    auto load_tile = [&](int kv0) {
        const int g0 = kv0 + wrow;
        if (g0 <= k_end) {                           // wave-uniform
            const bf16* kpg = kbase + page * kpp + k_col;
            const bf16* vpg = vbase + page * vpp + k_col;
#pragma unroll
            for (int it = 0; it < NLK; ++it) {
                // rows past k_end are never loaded: the index is clamped,
                // and stays inside the wave's 16 rows (g0 <= k_end)
                const int jc = min(g0 + it * RPI + k_r, k_end);
                kr[it] = *reinterpret_cast<const frag_ab*>(
                    kpg + (int64_t)(jc & page_mask) * kps);
            }
#pragma unroll
            for (int it = 0; it < NLV; ++it) {
                const int j = g0 + 2 * (it * RPI + k_r);
#pragma unroll
                for (int e = 0; e < 2; ++e)
                    vr[it][e] = *reinterpret_cast<const frag_ab*>(
                        vpg + (int64_t)(min(j + e, k_end) & page_mask) * vps);
            }
        } else {
            // zeros, not stale LDS: a masked weight is 0 and 0 * NaN is NaN
#pragma unroll
            for (int it = 0; it < NLK; ++it) kr[it] = frag_ab{};
#pragma unroll
            for (int it = 0; it < NLV; ++it) vr[it][0] = vr[it][1] = frag_ab{};
        }
        if (g0 + BLOCK_N <= k_end) page = page_of(g0 + BLOCK_N);
    };
    auto store_tile = [&]() {
#pragma unroll
        for (int it = 0; it < NLK; ++it) {
            const int row = wrow + it * RPI + k_r;
            *reinterpret_cast<frag_ab*>(&k_lds[row * KSTRIDE + k_col]) = kr[it];
        }
#pragma unroll
        for (int it = 0; it < NLV; ++it) {
            // V transposed; two rows at once -> 4-byte column stores
            const int row = wrow + 2 * (it * RPI + k_r);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                union { __bf16 h[2]; uint32_t u; } pair;
                pair.h[0] = vr[it][0][j];
                pair.h[1] = vr[it][1][j];
                *reinterpret_cast<uint32_t*>(
                    &vt_lds[(k_col + j) * VSTRIDE + row]) = pair.u;
            }
        }
    };

    load_tile(k_lo);
    for (int kv0 = k_lo; kv0 <= k_end; kv0 += BLOCK_N) {
        __syncthreads();               // every wave is done with the last tile
        store_tile();
        __syncthreads();
        if (kv0 + BLOCK_N <= k_end) load_tile(kv0 + BLOCK_N);   // in flight
        if (kv0 > pw_max) continue;    // wave-uniform: all masked for us

        // S = Q K^T for this wave's rows (16 x 64), exp2 domain, masked
        float s_tile[4][4];            // [nsub][reg]
        bool ok[4][4];
#pragma unroll
        for (int ns = 0; ns < 4; ++ns) {
            frag_cd acc = frag_cd{0.f, 0.f, 0.f, 0.f};
            __builtin_amdgcn_s_setprio(1);
#pragma unroll
            for (int c = 0; c < DCH; ++c) {
                frag_ab bK = *reinterpret_cast<const frag_ab*>(
                    &k_lds[(ns * 16 + lcol) * KSTRIDE + c * 32 + 8 * lgrp]);
                acc = MFMA_16x16x32(aQ[c], bK, acc);
            }
            __builtin_amdgcn_s_setprio(0);
            const int jk = kv0 + ns * 16 + lcol;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                ok[ns][r] = jk <= prow[r];
                s_tile[ns][r] = fmaf(slope2[r], (float)(jk - prow[r]),
                                     acc[r] * scale2);
            }
        }

        // online softmax; masking is a select on the score and the weight
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float mx = -FLT_MAX;
#pragma unroll
            for (int ns = 0; ns < 4; ++ns)
                mx = ok[ns][r] ? fmaxf(mx, s_tile[ns][r]) : mx;
#pragma unroll
            for (int off = 1; off < 16; off <<= 1)
                mx = fmaxf(mx, __shfl_xor(mx, off, WAVE_SIZE));
            const float m_new = fmaxf(m_run[r], mx);
            const float rescale = __builtin_amdgcn_exp2f(m_run[r] - m_new);
            m_run[r] = m_new;
            float ls = 0.f;
#pragma unroll
            for (int ns = 0; ns < 4; ++ns) {
                const float pv = ok[ns][r]
                    ? __builtin_amdgcn_exp2f(s_tile[ns][r] - m_new) : 0.f;
                ls += pv;
                p_lds[(4 * lgrp + r) * VSTRIDE + ns * 16 + lcol] = (bf16)pv;
            }
#pragma unroll
            for (int off = 1; off < 16; off <<= 1)
                ls += __shfl_xor(ls, off, WAVE_SIZE);
            l_run[r] = fmaf(l_run[r], rescale, ls);
#pragma unroll
            for (int s = 0; s < DSUB; ++s) accO[s][r] *= rescale;
        }
        wave_sync();                   // own-wave P writes before reads

        // O += P V  (64 keys in 2 chunks of 32)
#pragma unroll
        for (int kc = 0; kc < 2; ++kc) {
            frag_ab aP = *reinterpret_cast<const frag_ab*>(
                &p_lds[lcol * VSTRIDE + kc * 32 + 8 * lgrp]);
            __builtin_amdgcn_s_setprio(1);
#pragma unroll
            for (int ds = 0; ds < DSUB; ++ds) {
                frag_ab bV = *reinterpret_cast<const frag_ab*>(
                    &vt_lds[(ds * 16 + lcol) * VSTRIDE + kc * 32 + 8 * lgrp]);
                accO[ds] = MFMA_16x16x32(aP, bV, accO[ds]);
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
            bf16* orow = o + (int64_t)min(tok0 + ti, T - 1) * os
                + (int64_t)(h0 + (row & gmask)) * D;
#pragma unroll
            for (int ds = 0; ds < DSUB; ++ds)
                orow[ds * 16 + lcol] = (bf16)(live ? accO[ds][r] * inv_l : 0.f);
        }
    }
}

// One workgroup per (slot, y): merges the splits of the tile's real rows in
// split order; thread = (tile row, quarter of the 16-byte column groups).
template <int D>
__global__ __launch_bounds__(NW * WAVE_SIZE)
void paged_varlen_split_combine_kernel(const float* __restrict__ part_acc,
                                       const float* __restrict__ part_ml,
                                       const int* __restrict__ cu_q,
                                       bf16* __restrict__ o, int n_splits,
                                       int T, int B, int H, int gshift) {
    constexpr int NV = D / 16;      // float4 groups per thread
    const int wg = blockIdx.x, tid = threadIdx.x;
    const int tpt_shift = 6 - gshift;
    const int h0 = blockIdx.y << gshift;
    const TileId id = find_tile(cu_q, B, T, tpt_shift, wg, tid % WAVE_SIZE);
    if (id.seq < 0) {
        write_padding<D>(o, cu_at(cu_q, B, T), wg - id.total,
                         (int)gridDim.x - id.total, T, H, h0, gshift, tid);
        return;
    }
    const int c0 = cu_at(cu_q, id.seq, T);
    const int len = max(cu_at(cu_q, id.seq + 1, T) - c0, 0);
    const int i0 = id.tile << tpt_shift;
    const int n_tok = min(1 << tpt_shift, len - i0);
    const int row = tid >> 2, part = tid & 3;
    const int ti = row >> gshift;
    if (ti >= n_tok) return;

    float m = -FLT_MAX, l = 0.f;
    f32x4 a[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) a[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int s = 0; s < n_splits; ++s) {
        const int64_t wsrow =
            (((int64_t)wg * n_splits + s) * gridDim.y + blockIdx.y) * BLOCK_M
            + row;
        const float m2 = part_ml[2 * wsrow], l2 = part_ml[2 * wsrow + 1];
        if (l2 > 0.f) {             // a select: an empty split's acc is unwritten
            const float mn = fmaxf(m, m2);
            const float w1 = __builtin_amdgcn_exp2f(m - mn);
            const float w2 = __builtin_amdgcn_exp2f(m2 - mn);
            m = mn;
            l = l * w1 + l2 * w2;
            const f32x4* arow =
                reinterpret_cast<const f32x4*>(part_acc + wsrow * D);
#pragma unroll
            for (int i = 0; i < NV; ++i) a[i] = a[i] * w1 + arow[i * 4 + part] * w2;
        }
    }
    const float inv_l = l > 0.f ? 1.0f / l : 0.f;   // all empty: zeros
    bf16* orow = o + ((int64_t)min(c0 + i0 + ti, T - 1) * H
                      + h0 + (row & ((1 << gshift) - 1))) * D;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        bf16x4 out;
#pragma unroll
        for (int e = 0; e < 4; ++e) out[e] = (__bf16)(a[i][e] * inv_l);
        *reinterpret_cast<bf16x4*>(orow + (i * 4 + part) * 4) = out;
    }
}

}  // namespace

namespace decode_common {

// The host plan of the file header: shapes only.
SplitPlan make_split_plan(const char* op, int64_t T, int64_t B, int64_t H,
                          int64_t Hkv, int64_t capacity, int64_t forced) {
    TORCH_CHECK(T >= 1 && B >= 1 && Hkv >= 1 && H >= 1 && H % Hkv == 0 &&
                capacity >= 1, op, ": T, B, H, Hkv and the capacity must be "
                "positive, H a multiple of Hkv");
    TORCH_CHECK(forced >= 0 && forced <= MAX_SPLITS, op,
                ": n_splits must be 0 (auto) or 1..", MAX_SPLITS, ", got ",
                forced);
    // the GQA group shares a tile when it divides the 64 rows
    const int64_t G = H / Hkv;
    int gshift = 0;
    if (G == 2 || G == 4 || G == 8 || G == 16)
        while ((1 << gshift) < G) ++gshift;
    const int64_t gp = (int64_t)1 << gshift, tpt = BLOCK_M / gp;
    const int64_t n_slot = (T + tpt - 1) / tpt + B, ny = H / gp;
    int64_t n = forced;
    if (n == 0) {
        n = (TARGET_WGS + n_slot * ny - 1) / (n_slot * ny);
        n = std::min<int64_t>(n, std::min<int64_t>(MAX_SPLITS,
                                                   capacity / BLOCK_N));
        n = std::max<int64_t>(n, 1);
    }
    return {(int)n, gshift, n_slot, ny};
}

void launch_split_combine(const float* part_acc, const float* part_ml,
                          const int* cu_q, __hip_bfloat16* o,
                          const SplitPlan& plan, int64_t T, int64_t B,
                          int64_t H, int64_t D) {
    auto stream = at::cuda::getCurrentCUDAStream();
    const dim3 grid((unsigned)plan.n_slot, (unsigned)plan.ny);
    auto launch = [&](auto dv_) {
        constexpr int DV = decltype(dv_)::value;
        hipLaunchKernelGGL((paged_varlen_split_combine_kernel<DV>), grid,
                           dim3(NW * WAVE_SIZE), 0, stream, part_acc, part_ml,
                           cu_q, o, plan.n_splits, (int)T, (int)B, (int)H,
                           plan.gshift);
    };
    if (D == 64) launch(std::integral_constant<int, 64>{});
    else launch(std::integral_constant<int, 128>{});
}

}  // namespace decode_common

std::tuple<int64_t, int64_t> paged_varlen_split_plan(int64_t T, int64_t B,
                                                     int64_t H, int64_t Hkv,
                                                     int64_t capacity) {
    const SplitPlan p = decode_common::make_split_plan(
        "paged_varlen_split_attn", T, B, H, Hkv, capacity, 0);
    return {p.n_splits, p.n_slot};
}

torch::Tensor paged_varlen_split_attn(torch::Tensor q, torch::Tensor k_pool,
                                      torch::Tensor v_pool,
                                      torch::Tensor block_table,
                                      torch::Tensor slopes, double scale,
                                      torch::Tensor cu_q, torch::Tensor start,
                                      int64_t n_splits, bool short_body) {
    using namespace attn_checks;
    const char* op = "paged_varlen_split_attn";
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
    const int shift = check_paged(op, k_pool, v_pool, block_table, B, D,
                                  q.device());
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

    const SplitPlan plan =
        decode_common::make_split_plan(op, T, B, H, Hkv, capacity, n_splits);
    TORCH_CHECK(plan.ny <= 65535, op, ": H must fit a grid dimension");
    const int64_t ws_rows = plan.n_slot * plan.n_splits * plan.ny * BLOCK_M;
    TORCH_CHECK(plan.n_splits == 1 || ws_rows * (D + 2) * 4 <= MAX_WORKSPACE,
                op, ": n_splits = ", plan.n_splits, " needs a workspace of ",
                ws_rows * (D + 2) * 4, " bytes, more than ", MAX_WORKSPACE,
                "; use fewer splits");

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
        hipLaunchKernelGGL((paged_varlen_split_attn_kernel<DV, SP>), grid,
                           dim3(NW * WAVE_SIZE), 0, stream,
                           reinterpret_cast<const bf16*>(q.data_ptr()),
                           reinterpret_cast<const bf16*>(k_pool.data_ptr()),
                           reinterpret_cast<const bf16*>(v_pool.data_ptr()),
                           block_table.data_ptr<int>(), block_table.stride(0),
                           slopes.data_ptr<float>(), (float)scale,
                           cu_q.data_ptr<int>(),
                           start.data_ptr<int64_t>(), (int)start.numel(),
                           reinterpret_cast<bf16*>(o.data_ptr()), acc_p, ml_p,
                           (int)T, (int)B, (int)H, (int)(H / Hkv), plan.gshift,
                           (int)short_body,
                           (int)capacity, (int)n_pages, shift,
                           q.stride(0), q.stride(1),
                           k_pool.stride(0), k_pool.stride(1), k_pool.stride(2),
                           v_pool.stride(0), v_pool.stride(1),
                           v_pool.stride(2));
        if constexpr (SP)
            decode_common::launch_split_combine(
                acc_p, ml_p, cu_q.data_ptr<int>(),
                reinterpret_cast<bf16*>(o.data_ptr()), plan, T, B, H, D);
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
