// Ragged-batch paged attention for gfx950: one launch over a TOKEN-PACKED
// batch.  Sequence b owns the packed rows cu_q[b] .. cu_q[b+1]-1 of q [T,H,D];
// row t of sequence b sits at p = start[b] + (t - cu_q[b]) and sees keys 0..p
// of sequence b, read from the page pools through block_table[b].
//
//   o[t,h,:] = softmax_j( scale * q[t,h,:]·K[b,h/G,j,:] + slopes[h]*(j - p) )
//              @ V[b,h/G,j,:]           j in [0, p]
//   K[b,hk,j,:] = k_pool[clamp(block_table[b, j / PAGE], 0, n_pages-1),
//                        hk, j % PAGE, :]                     (V likewise)
//
// Operands: q [T,H,D] bf16, any strides with d contiguous and 16-byte rows;
// pools, block_table [B,max_pages] and slopes as for paged_prefill_attn
// (paged_prefill_attention.hip); cu_q int32 [B+1] and start int64 [B] (or one
// element for all), both READ ON THE DEVICE.  o is [T,H,D], contiguous.  Rows
// t >= cu_q[B] are padding and give zeros, rows with p outside
// [0, max_pages*PAGE) give zeros, a sequence may own zero rows.  The caller
// has already written the rows' own K/V into the pools.
//
// Work split (shapes only, so the call is graph-capturable).  A workgroup is
// 4 waves x 16 rows of a 64-row M tile, v_mfma_f32_16x16x32_bf16, and the 64
// rows are TPT = 64/gp tokens x gp heads of ONE kv head: gp = G when G is in
// {1,2,4,8,16}, else 1.  Tile row r is token r >> log2(gp) and head
// h0 + (r & (gp-1)), h0 = blockIdx.y * gp, so one staged K/V tile serves the
// whole GQA group and position, causal cut and slope are per-row quantities
// (4 per lane in the C layout).  A tile never crosses a sequence boundary:
// sum_b ceil(len_b/TPT) <= ceil(T/TPT) + B, which is the grid's x extent, and
// each workgroup finds its (b, tile within b) from cu_q itself: every wave
// scans the per-sequence tile counts 64 sequences at a time (shuffle prefix
// sum, ballot for the first sequence whose running total passes blockIdx.x).
// The scan is B/64 steps of a few instructions on data that sits in L2, so
// it needs no prep kernel and no tile map; B <= MAX_SEQS = 1024 and
// T <= MAX_TOKENS = 2^20 (checked on the host) keep every sum below 2^31.
// The workgroups left over after the last tile write the zeros of the
// padding rows, strided over their count, and load nothing else.
//
// The rest is the structure of paged_prefill_attention.hip: 64-key tiles
// staged through LDS (K row-major on padded rows, V transposed), P bounced
// through LDS from C- to A-layout, fp32 online softmax in the exp2 domain with
// select-masking, tile t+1 fetched into registers while tile t is computed,
// wave-uniform table lookups one tile ahead.
//
// What is never read.  p_max is the largest in-range position of the
// workgroup's real rows; the key loop runs p_max/64 + 1 tiles, row indices
// are clamped to p_max, a wave whose 16 staged rows start beyond p_max loads
// nothing and stages zeros, table entries with index > p_max / PAGE are never
// read, every id read is clamped into [0, n_pages-1].  cu_q is device data:
// every value read from it is clamped into [0, T], so lengths lie in [0, T]
// and every token index in [0, T-1]; a corrupt cu_q gives wrong numbers (rows
// left unwritten included), never an out-of-bounds access.
//
// No atomics, no split-KV: results are bit-reproducible for fixed inputs.
//
// Resources (hipcc -O3 --offload-arch=gfx950
// -Rpass-analysis=kernel-resource-usage):
//   D = 64 : 133 VGPRs + 16 AGPRs, 75 SGPRs, 27648 B LDS, 3 waves/SIMD
//   D = 128: 175 VGPRs + 32 AGPRs, 75 SGPRs, 45056 B LDS, 2 waves/SIMD
// no scratch at either head dim.
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

#include <cfloat>
#include <type_traits>

#include "attn_checks.h"
#include "mfma_frag.h"

namespace {

constexpr int BLOCK_M = 64;   // (token, head) rows per workgroup
constexpr int BLOCK_N = 64;   // keys per LDS tile
constexpr int NW = 4;         // waves per workgroup, 16 rows each
constexpr int PAD = 8;        // bf16 elements (16 B) of row padding in LDS
constexpr int MAX_SEQS = 1024;
constexpr int MAX_TOKENS = 1 << 20;
constexpr float LOG2E = 1.4426950408889634f;

template <int D>
__global__ __launch_bounds__(NW * WAVE_SIZE)
void paged_varlen_attn_kernel(const bf16* __restrict__ q,
                              const bf16* __restrict__ k_pool,
                              const bf16* __restrict__ v_pool,
                              const int* __restrict__ block_table,
                              int64_t bt_stride,
                              const float* __restrict__ slopes, float scale,
                              const int* __restrict__ cu_q,
                              const int64_t* __restrict__ start, int start_n,
                              bf16* __restrict__ o,           // [T,H,D]
                              int T, int B, int H, int G, int gshift,
                              int capacity, int n_pages, int page_shift,
                              int64_t qt, int64_t qh,
                              int64_t kpp, int64_t kph, int64_t kps,
                              int64_t vpp, int64_t vph, int64_t vps) {
    constexpr int DCH = D / 32;     // K-chunks per QK^T mfma row
    constexpr int DSUB = D / 16;    // output d-subtiles
    constexpr int KSTRIDE = D + PAD;
    constexpr int VSTRIDE = BLOCK_N + PAD;
    constexpr int TPR = D / 8;      // 16-byte packets per row
    constexpr int NLK = 16 * TPR / WAVE_SIZE;   // K loads per lane and tile
    constexpr int NLV = 8 * TPR / WAVE_SIZE;    // V row-pair loads per lane

    __shared__ bf16 k_lds[BLOCK_N * KSTRIDE];
    __shared__ bf16 vt_lds[D * VSTRIDE];
    __shared__ bf16 p_lds[NW][16 * VSTRIDE];

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

    auto cu = [&](int i) { return min(max(cu_q[i], 0), T); };

    // ---- which (sequence, tile) is this workgroup?  Every wave scans alone:
    // the results are wave-uniform and equal in all four
    int total = 0, seq = -1, tile = 0;
    for (int base = 0; base < B; base += WAVE_SIZE) {
        const int b = base + lane;
        int n = 0;
        if (b < B) n = (max(cu(b + 1) - cu(b), 0) + TPT - 1) >> tpt_shift;
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
    seq = __builtin_amdgcn_readfirstlane(seq);
    tile = __builtin_amdgcn_readfirstlane(tile);
    total = __builtin_amdgcn_readfirstlane(total);

    if (seq < 0) {
        // past the last tile: the zeros of the padding rows, strided over
        // the surplus workgroups; each thread one 16-byte packet at a time
        const int n_surplus = (int)gridDim.x - total;
        const int row = tid >> 2;               // tile row 0..63
        const int head = h0 + (row & gmask);
        for (int64_t t = (int64_t)cu(B) + (int64_t)(wg - total) * TPT
                 + (row >> gshift);
             t < T; t += (int64_t)n_surplus * TPT) {
            bf16* orow = o + t * os + (int64_t)head * D;
            for (int c = (tid & 3) * 8; c < D; c += 32)
                *reinterpret_cast<frag_ab*>(orow + c) = frag_ab{};
        }
        return;
    }

    const int c0 = cu(seq);
    const int len = max(cu(seq + 1) - c0, 0);
    const int i0 = tile << tpt_shift;           // first row of the tile in seq
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
    const int wr0 = wave * 16;                  // this wave's first tile row

    if (p_lo > p_max) {
        // no row of the tile is in range: zeros, and nothing is loaded
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = wr0 + 4 * lgrp + r;
            const int ti = row >> gshift;
            if (ti < n_tok) {
                bf16* orow = o + (int64_t)min(tok0 + ti, T - 1) * os
                    + (int64_t)(h0 + (row & gmask)) * D;
#pragma unroll
                for (int ds = 0; ds < DSUB; ++ds)
                    orow[ds * 16 + lcol] = (bf16)0.f;
            }
        }
        return;
    }

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
        return min(max(id, 0), n_pages - 1);
    };
    const bf16* kbase = k_pool + hk * kph;
    const bf16* vbase = v_pool + hk * vph;
    const int wrow = __builtin_amdgcn_readfirstlane(wave * 16);
    const int k_r = lane / TPR, k_col = (lane % TPR) * 8;   // + it*(64/TPR) rows

    frag_ab kr[NLK], vr[NLV][2];
    int page = 0;
    if (wrow <= p_max) page = page_of(wrow);

    // fetch the wave's part of the tile at kv0 into registers, then the page
    // id of the NEXT tile if the wave will load there
    auto load_tile = [&](int kv0) {
        const int g0 = kv0 + wrow;
        if (g0 <= p_max) {                           // wave-uniform
            const bf16* kpg = kbase + page * kpp + k_col;
            const bf16* vpg = vbase + page * vpp + k_col;
#pragma unroll
            for (int it = 0; it < NLK; ++it) {
                // rows past p_max are never loaded: the index is clamped,
                // and stays inside the wave's 16 rows (g0 <= p_max)
                const int jc = min(g0 + it * (WAVE_SIZE / TPR) + k_r, p_max);
                kr[it] = *reinterpret_cast<const frag_ab*>(
                    kpg + (int64_t)(jc & page_mask) * kps);
            }
#pragma unroll
            for (int it = 0; it < NLV; ++it) {
                const int j = g0 + 2 * (it * (WAVE_SIZE / TPR) + k_r);
#pragma unroll
                for (int e = 0; e < 2; ++e)
                    vr[it][e] = *reinterpret_cast<const frag_ab*>(
                        vpg + (int64_t)(min(j + e, p_max) & page_mask) * vps);
            }
        } else {
            // zeros, not stale LDS: a masked weight is 0 and 0 * NaN is NaN
#pragma unroll
            for (int it = 0; it < NLK; ++it) kr[it] = frag_ab{};
#pragma unroll
            for (int it = 0; it < NLV; ++it) vr[it][0] = vr[it][1] = frag_ab{};
        }
        if (g0 + BLOCK_N <= p_max) page = page_of(g0 + BLOCK_N);
    };
    auto store_tile = [&]() {
#pragma unroll
        for (int it = 0; it < NLK; ++it) {
            const int row = wrow + it * (WAVE_SIZE / TPR) + k_r;
            *reinterpret_cast<frag_ab*>(&k_lds[row * KSTRIDE + k_col]) = kr[it];
        }
#pragma unroll
        for (int it = 0; it < NLV; ++it) {
            // V transposed; two rows at once -> 4-byte column stores
            const int row = wrow + 2 * (it * (WAVE_SIZE / TPR) + k_r);
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

    const int n_tiles = p_max / BLOCK_N + 1;
    load_tile(0);
    for (int t = 0; t < n_tiles; ++t) {
        const int kv0 = t * BLOCK_N;
        __syncthreads();               // every wave is done with tile t-1
        store_tile();
        __syncthreads();
        if (t + 1 < n_tiles) load_tile(kv0 + BLOCK_N);   // in flight below
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
                p_lds[wave][(4 * lgrp + r) * VSTRIDE + ns * 16 + lcol] =
                    (bf16)pv;
            }
#pragma unroll
            for (int off = 1; off < 16; off <<= 1)
                ls += __shfl_xor(ls, off, WAVE_SIZE);
            l_run[r] = fmaf(l_run[r], rescale, ls);
#pragma unroll
            for (int s = 0; s < DSUB; ++s) accO[s][r] *= rescale;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();   // own-wave P writes before reads
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

        // O += P V  (64 keys in 2 chunks of 32)
#pragma unroll
        for (int kc = 0; kc < 2; ++kc) {
            frag_ab aP = *reinterpret_cast<const frag_ab*>(
                &p_lds[wave][lcol * VSTRIDE + kc * 32 + 8 * lgrp]);
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

    // epilogue: real rows only; out-of-range positions give zeros
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = wr0 + 4 * lgrp + r;
        const int ti = row >> gshift;
        if (ti >= n_tok) continue;
        const bool in_range = prow[r] >= 0 && prow[r] < capacity;
        const float inv_l = in_range ? 1.0f / l_run[r] : 0.f;
        bf16* orow = o + (int64_t)min(tok0 + ti, T - 1) * os
            + (int64_t)(h0 + (row & gmask)) * D;
#pragma unroll
        for (int ds = 0; ds < DSUB; ++ds)
            orow[ds * 16 + lcol] =
                (bf16)(in_range ? accO[ds][r] * inv_l : 0.f);
    }
}

}  // namespace

torch::Tensor paged_varlen_attn(torch::Tensor q, torch::Tensor k_pool,
                                torch::Tensor v_pool,
                                torch::Tensor block_table,
                                torch::Tensor slopes, double scale,
                                torch::Tensor cu_q, torch::Tensor start) {
    using namespace attn_checks;
    const char* op = "paged_varlen_attn";
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

    // the GQA group shares a tile when it divides the 64 rows
    const int64_t G = H / Hkv;
    int gshift = 0;
    if (G == 2 || G == 4 || G == 8 || G == 16)
        while ((1 << gshift) < G) ++gshift;
    const int64_t gp = (int64_t)1 << gshift, tpt = BLOCK_M / gp;
    TORCH_CHECK(H / gp <= 65535, op, ": H must fit a grid dimension");

    auto o = torch::empty({T, H, D}, q.options());
    auto stream = at::cuda::getCurrentCUDAStream();
    auto launch = [&](auto dv_) {
        constexpr int DV = decltype(dv_)::value;
        hipLaunchKernelGGL((paged_varlen_attn_kernel<DV>),
                           dim3((unsigned)((T + tpt - 1) / tpt + B),
                                (unsigned)(H / gp)),
                           dim3(NW * WAVE_SIZE), 0, stream,
                           reinterpret_cast<const bf16*>(q.data_ptr()),
                           reinterpret_cast<const bf16*>(k_pool.data_ptr()),
                           reinterpret_cast<const bf16*>(v_pool.data_ptr()),
                           block_table.data_ptr<int>(), block_table.stride(0),
                           slopes.data_ptr<float>(), (float)scale,
                           cu_q.data_ptr<int>(),
                           start.data_ptr<int64_t>(), (int)start.numel(),
                           reinterpret_cast<bf16*>(o.data_ptr()),
                           (int)T, (int)B, (int)H, (int)G, gshift,
                           (int)capacity, (int)n_pages, shift,
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
