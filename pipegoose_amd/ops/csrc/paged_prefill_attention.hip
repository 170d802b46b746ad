// Paged prefill attention for gfx950: Sq >= 1 query rows per sequence at
// positions start[b] .. start[b]+Sq-1 against keys 0 .. position, every key
// read from the page pools through the block table (chunked prefill, prefix
// reuse).  Causal cut, ALiBi bias and the GQA head mapping are in-kernel.
//
//   o[b,h,i,:] = softmax_j( scale * q[b,h,i,:]·K[b,h/G,j,:]
//                           + slopes[h]*(j - p_i) ) @ V[b,h/G,j,:]
//                j in [0, p_i],  p_i = start[b] + i,  i in [0, Sq)
//   K[b,hk,j,:] = k_pool[clamp(block_table[b, j / PAGE], 0, n_pages-1),
//                        hk, j % PAGE, :]                     (V likewise)
//
// Operands as in paged_decode_attn (decode_attention.hip): q [B,H,Sq,D] bf16,
// any strides with d contiguous and 16-byte rows; pools [n_pages,Hkv,PAGE,D],
// PAGE in {16,32,64,128}, D in {64,128}; block_table int32 [B,max_pages], row
// stride free; slopes fp32 [H]; `start` int64 with 1 or B elements, READ ON
// THE DEVICE.  The launch plan is shapes only (grid (ceil(Sq/64), H, B)), so
// the call is graph-capturable with the positions and the table as data.  The
// result is physically [B,Sq,H,D] and returned as the [B,H,Sq,D] view.  The
// caller has already written the chunk's own K/V into the pools
// (paged_kv_write): everything is read from the pools.
//
// Structure: the v1 forward of attention.hip.  One workgroup = 4 waves x 16
// query rows, v_mfma_f32_16x16x32_bf16; 64-key tiles staged through LDS (K
// row-major on padded rows, V transposed), P bounced through LDS from C- to
// A-layout, fp32 online softmax in the exp2 domain with l summed from the fp32
// weights.  Tile t+1 is fetched into registers while tile t is computed.  A
// wave stages rows [16w, 16w+16) of a tile: 16-aligned, so inside ONE page for
// every allowed PAGE, and the table lookup is wave-uniform (one scalar load
// per wave and tile, fetched one tile ahead), as in the decode kernel.
//
// What is never read.  p_max is the largest in-range position of the
// workgroup's rows.  The key loop runs p_max/64 + 1 tiles (data, not shape);
// row indices are clamped to p_max; a wave whose 16 rows start beyond p_max
// loads nothing and stages zeros; table entries with index > p_max / PAGE are
// never read; every id read is clamped into [0, n_pages-1].  So slots beyond
// may hold any bits, and a corrupt table gives wrong numbers, never an
// out-of-bounds access.  start[b] + Sq <= max_pages*PAGE cannot be checked on
// the host: rows whose position is outside [0, max_pages*PAGE) get an
// all-zero output row (paged_kv_write drops the same rows) and take no part
// in p_max; a workgroup with no in-range row loads nothing at all.
//
// Masking is a select on the score and on the weight; the running maximum
// starts at -FLT_MAX, and every in-range row sees key 0 in the first tile, so
// no (-inf)-(-inf) or 0/0 arises.  No atomics, no split-KV: results are
// bit-reproducible for fixed inputs.
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

#include <cfloat>
#include <type_traits>

#include "attn_checks.h"
#include "mfma_frag.h"

namespace {

constexpr int BLOCK_M = 64;   // query rows per workgroup
constexpr int BLOCK_N = 64;   // keys per LDS tile
constexpr int NW = 4;         // waves per workgroup, 16 query rows each
constexpr int PAD = 8;        // bf16 elements (16 B) of row padding in LDS
constexpr float LOG2E = 1.4426950408889634f;

template <int D>
__global__ __launch_bounds__(NW * WAVE_SIZE)
void paged_prefill_attn_kernel(const bf16* __restrict__ q,
                               const bf16* __restrict__ k_pool,
                               const bf16* __restrict__ v_pool,
                               const int* __restrict__ block_table,
                               int64_t bt_stride,
                               const float* __restrict__ slopes, float scale,
                               const int64_t* __restrict__ start, int start_n,
                               bf16* __restrict__ o,          // [B,Sq,H,D]
                               int H, int G, int Sq, int capacity,
                               int n_pages, int page_shift,
                               int64_t qb, int64_t qh, int64_t qs,
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

    const int qblock = blockIdx.x;
    const int h = blockIdx.y;
    const int b = blockIdx.z;
    const int tid = threadIdx.x;
    const int wave = tid / WAVE_SIZE;
    const int lane = tid % WAVE_SIZE;
    const int lgrp = lane >> 4;       // 0..3
    const int lcol = lane & 15;       // 0..15
    const int hk = h / G;

    // capacity and Sq are < 2^30: a start below -2^30 or at or above capacity
    // puts every row out of range either way, and clamped to that interval
    // all the int arithmetic below is exact
    int64_t st64 = start[start_n == 1 ? 0 : b];
    st64 = st64 < -((int64_t)1 << 30) ? -((int64_t)1 << 30) : st64;
    const int st = (int)(st64 > capacity ? capacity : st64);

    const int i0 = qblock * BLOCK_M;                 // first row of the block
    const int i_last = min(i0 + BLOCK_M, Sq) - 1;    // last REAL row
    const int p_lo = max(st + i0, 0);
    const int p_max = min(st + i_last, capacity - 1);

    const int64_t os = (int64_t)H * D;
    bf16* op = o + ((int64_t)b * Sq * H + h) * D;
    const int wi0 = i0 + wave * 16;                  // this wave's first row

    if (p_lo > p_max) {
        // no row of the block is in range: zeros, and nothing is loaded
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = wi0 + 4 * lgrp + r;
            if (i < Sq) {
#pragma unroll
                for (int ds = 0; ds < DSUB; ++ds)
                    op[i * os + ds * 16 + lcol] = (bf16)0.f;
            }
        }
        return;
    }

    // the largest in-range position of this wave's rows (-1: none): tiles
    // that start beyond it are wholly masked for the wave
    const int pw_max =
        wi0 < Sq ? min(st + min(wi0 + 15, Sq - 1), capacity - 1) : -1;

    frag_ab aQ[DCH];
    {
        // a ragged last block clamps its loads to row Sq-1
        const bf16* qrow = q + b * qb + h * qh
            + (int64_t)min(wi0 + lcol, Sq - 1) * qs;
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
                s_tile[ns][r] = fmaf(slope2, (float)(jk - prow[r]),
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
        const int i = wi0 + 4 * lgrp + r;
        if (i >= Sq) continue;
        const bool in_range = prow[r] >= 0 && prow[r] < capacity;
        const float inv_l = in_range ? 1.0f / l_run[r] : 0.f;
        bf16* orow = op + i * os;
#pragma unroll
        for (int ds = 0; ds < DSUB; ++ds)
            orow[ds * 16 + lcol] =
                (bf16)(in_range ? accO[ds][r] * inv_l : 0.f);
    }
}

}  // namespace

torch::Tensor paged_prefill_attn(torch::Tensor q, torch::Tensor k_pool,
                                 torch::Tensor v_pool,
                                 torch::Tensor block_table,
                                 torch::Tensor slopes, double scale,
                                 torch::Tensor start) {
    using namespace attn_checks;
    const char* op = "paged_prefill_attn";
    TORCH_CHECK(q.dim() == 4 && q.size(2) >= 1, op,
                ": q must be [B, H, Sq, D] with Sq >= 1");
    const int64_t B = q.size(0), H = q.size(1), Sq = q.size(2), D = q.size(3);
    check_operand(op, "q", q, {B, H, Sq, D});
    const int shift = check_paged(op, k_pool, v_pool, block_table, B, D,
                                  q.device());
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
        hipLaunchKernelGGL((paged_prefill_attn_kernel<DV>),
                           dim3((unsigned)((Sq + BLOCK_M - 1) / BLOCK_M),
                                (unsigned)H, (unsigned)B),
                           dim3(NW * WAVE_SIZE), 0, stream,
                           reinterpret_cast<const bf16*>(q.data_ptr()),
                           reinterpret_cast<const bf16*>(k_pool.data_ptr()),
                           reinterpret_cast<const bf16*>(v_pool.data_ptr()),
                           block_table.data_ptr<int>(), block_table.stride(0),
                           slopes.data_ptr<float>(), (float)scale,
                           start.data_ptr<int64_t>(), (int)start.numel(),
                           reinterpret_cast<bf16*>(o_phys.data_ptr()),
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
