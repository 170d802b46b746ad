// Flash attention (causal + ALiBi) for gfx950 — hand-written CDNA4 MFMA.
//
// The ALiBi bias slope*(j-i) and the causal mask are computed IN-KERNEL from
// per-head slopes, so no [H,S,S] bias tensor is materialized or re-read from
// HBM (that tensor dominated the sdpa-with-bias path's memory traffic).
// Online softmax (flash2) with fp32 running stats; the backward is two-pass
// (kv-outer dK/dV, q-outer dQ, plus a tiny delta = rowsum(dO*O) kernel),
// recomputes P from (q, k, lse) and uses no atomics.  Tensors are [B,H,S,D]
// logical with arbitrary strides (d contiguous); kv_off shifts the kv
// positions (ring-attention blocks), key j is visible to row i when
// j + kv_off <= i:  <= -S fully visible, (-S, 0) shifted causal (masked
// elementwise, any integer), 0 causal; a positive one is rejected by the
// host check (its first rows would see no key at all).
//
// Two kernel families; select_variant() in the host section at the end of
// this file (bound as attn_variant) is the one place that picks, for the
// forward and the backward alike (D in {64,128}, S % 64 == 0):
//
//   S % 128 == 64  v1, 4 waves   fwd grid S/64;  bwd: delta, dkdv, dq
//   S % 256 == 128 v2, 4 waves   fwd grid S/128; bwd: delta, dq_v2, dkdv_v2
//   S % 256 == 0   v2, 8 waves   fwd grid S/256; bwd: delta, dq_v2, dkdv_v2
//
// v2 is the design (every shape the models and the benchmark use):
// v_mfma_f32_32x32x16_bf16, a wave owns 32 rows, "swapped" products
// (St = K·Q^T, O^T = V^T·P^T) so that a lane owns one q row and softmax
// statistics are lane-local, XOR-swizzled and sub-tiled LDS images read with
// ds_read_b64_tr_b16, double-buffered tiles, exp2 domain.  dkdv_v2 is one
// fused kernel at D=64; at D=128 it would spill and runs as a dv-only pass
// plus two half-width dk passes.
//
// v1 is the fallback for S % 128 == 64, which v2's 128-row workgroups cannot
// tile: v_mfma_f32_16x16x32_bf16, one workgroup = 4 waves x 16 rows = 64 q
// (or kv) rows, padded LDS rows, P bounced through LDS from C- to A-layout,
// 16-lane shuffle reductions for the row statistics.
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

#include <string>
#include <tuple>
#include <type_traits>

#include "mfma_frag.h"

// ======================================================================
// v1 forward: 4 waves x 16 q rows.  K/V tiles (64 rows) stage through LDS; V
// is stored transposed so the P·V MFMA's B-fragment reads are contiguous 16B.
namespace {

constexpr int BLOCK_M = 64;   // v1: q (or kv) rows per workgroup
constexpr int BLOCK_N = 64;   // kv rows per LDS tile
constexpr int NWAVES = 4;     // v1: BLOCK_M / 16
constexpr int PAD = 8;        // bf16 elements (16 B) of row padding in LDS
constexpr float NEG_INF = -1e30f;

template <int D>
__global__ __launch_bounds__(NWAVES * WAVE_SIZE)
void attn_fwd_kernel(const bf16* __restrict__ q, const bf16* __restrict__ k,
                     const bf16* __restrict__ v,
                     const float* __restrict__ slopes, float scale,
                     bf16* __restrict__ o, float* __restrict__ lse,
                     int B, int H, int S, int kv_off, int kv_group,
                     int64_t qb, int64_t qh, int64_t qs,
                     int64_t kb, int64_t kh, int64_t ks,
                     int64_t vb, int64_t vh, int64_t vs,
                     int64_t ob, int64_t oh, int64_t os) {
    // Tensors are [B, H, S, D] LOGICAL with arbitrary strides (d contiguous):
    // the model's qkv views come straight from the fused projection with no
    // .contiguous() copies (those copies were ~6% of the training step).
    constexpr int DCH = D / 32;    // K-chunks per QK^T mfma row
    constexpr int DSUB = D / 16;   // output d-subtiles
    constexpr int KSTRIDE = D + PAD;
    constexpr int VSTRIDE = BLOCK_N + PAD;
    constexpr int NT = NWAVES * WAVE_SIZE;

    __shared__ bf16 k_lds[BLOCK_N * KSTRIDE];
    __shared__ bf16 vt_lds[D * VSTRIDE];
    __shared__ bf16 p_lds[NWAVES][16 * VSTRIDE];

    const int qblock = blockIdx.x;
    const int h = blockIdx.y;
    const int b = blockIdx.z;
    const int tid = threadIdx.x;
    const int wave = tid / WAVE_SIZE;
    const int lane = tid % WAVE_SIZE;
    const int lgrp = lane >> 4;       // 0..3
    const int lcol = lane & 15;       // 0..15

    const int64_t bh_off = ((int64_t)b * H + h) * S;  // lse layout
    const int hk = h / kv_group;  // GQA: q heads share kv heads
    const bf16* qp = q + b * qb + h * qh;
    const bf16* kp = k + b * kb + hk * kh;
    const bf16* vp = v + b * vb + hk * vh;
    bf16* op = o + b * ob + h * oh;

    // wave owns rows [qrow0, qrow0 + 16)
    const int qrow0 = qblock * BLOCK_M + wave * 16;
    const float slope = slopes[h];

    frag_ab aQ[DCH];
    {
        const bf16* qrow = qp + (int64_t)(qrow0 + lcol) * qs;
#pragma unroll
        for (int c = 0; c < DCH; ++c) {
            aQ[c] = *reinterpret_cast<const frag_ab*>(qrow + c * 32 + 8 * lgrp);
        }
    }

    frag_cd accO[DSUB];
    float m_run[4], l_run[4];
#pragma unroll
    for (int s = 0; s < DSUB; ++s) accO[s] = frag_cd{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int r = 0; r < 4; ++r) { m_run[r] = NEG_INF; l_run[r] = 0.f; }

    // kv positions are globally shifted by kv_off (ring attention blocks):
    // kv_off <= -S means every kv position is visible (no causal cut)
    int n_kv_blocks = (kv_off <= -S) ? (S / BLOCK_N)
        : (qblock * BLOCK_M + BLOCK_M - kv_off + BLOCK_N - 1) / BLOCK_N;
    n_kv_blocks = min(max(n_kv_blocks, 0), S / BLOCK_N);
    for (int nb = 0; nb < n_kv_blocks; ++nb) {
        const int kvrow0 = nb * BLOCK_N;
        __syncthreads();
        {   // cooperative K tile load (row-major, 16B packets)
            constexpr int PACKETS = BLOCK_N * D / 8;
            for (int p = tid; p < PACKETS; p += NT) {
                const int row = p / (D / 8);
                const int col = (p % (D / 8)) * 8;
                *reinterpret_cast<frag_ab*>(&k_lds[row * KSTRIDE + col]) =
                    *reinterpret_cast<const frag_ab*>(
                        kp + (int64_t)(kvrow0 + row) * ks + col);
            }
        }
        {   // V tile load, transposed; two rows at once -> 4 B column stores
            constexpr int PACKETS = (BLOCK_N / 2) * (D / 8);
            for (int p = tid; p < PACKETS; p += NT) {
                const int row = (p / (D / 8)) * 2;
                const int col = (p % (D / 8)) * 8;
                frag_ab p0 = *reinterpret_cast<const frag_ab*>(
                    vp + (int64_t)(kvrow0 + row) * vs + col);
                frag_ab p1 = *reinterpret_cast<const frag_ab*>(
                    vp + (int64_t)(kvrow0 + row + 1) * vs + col);
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    union { __bf16 h[2]; uint32_t u; } pair;
                    pair.h[0] = p0[j];
                    pair.h[1] = p1[j];
                    *reinterpret_cast<uint32_t*>(&vt_lds[(col + j) * VSTRIDE + row]) = pair.u;
                }
            }
        }
        __syncthreads();

        // S = Q K^T for this wave's rows (16 x 64)
        float s_tile[4][4];  // [nsub][reg]
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
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int iq = qrow0 + 4 * lgrp + r;
                const int jk = kvrow0 + ns * 16 + lcol + kv_off;
                float sv = acc[r] * scale + slope * (float)(jk - iq);
                s_tile[ns][r] = (jk <= iq) ? sv : NEG_INF;
            }
        }

        // online softmax update
        float m_new[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float mx = fmaxf(fmaxf(s_tile[0][r], s_tile[1][r]),
                             fmaxf(s_tile[2][r], s_tile[3][r]));
#pragma unroll
            for (int off = 1; off < 16; off <<= 1) {
                mx = fmaxf(mx, __shfl_xor(mx, off, WAVE_SIZE));
            }
            m_new[r] = fmaxf(m_run[r], mx);
        }
        float rescale[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            rescale[r] = __expf(m_run[r] - m_new[r]);
            m_run[r] = m_new[r];
            l_run[r] *= rescale[r];
        }
#pragma unroll
        for (int s = 0; s < DSUB; ++s) {
#pragma unroll
            for (int r = 0; r < 4; ++r) accO[s][r] *= rescale[r];
        }

        // P = exp(S - m); stage bf16 for the PV mfma; accumulate l
#pragma unroll
        for (int ns = 0; ns < 4; ++ns) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float pv = __expf(s_tile[ns][r] - m_run[r]);
                s_tile[ns][r] = pv;
                p_lds[wave][(4 * lgrp + r) * VSTRIDE + ns * 16 + lcol] = (bf16)pv;
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float ls = s_tile[0][r] + s_tile[1][r] + s_tile[2][r] + s_tile[3][r];
#pragma unroll
            for (int off = 1; off < 16; off <<= 1) {
                ls += __shfl_xor(ls, off, WAVE_SIZE);
            }
            l_run[r] += ls;
        }
        __builtin_amdgcn_s_waitcnt(0);  // own-wave P writes visible

        // O += P V  (K = 64 in 2 chunks of 32)
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

    // epilogue
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int iq = qrow0 + 4 * lgrp + r;
        const float inv_l = 1.0f / l_run[r];
        bf16* orow = op + (int64_t)iq * os;
#pragma unroll
        for (int ds = 0; ds < DSUB; ++ds) {
            orow[ds * 16 + lcol] = (bf16)(accO[ds][r] * inv_l);
        }
        if (lcol == 0) {
            lse[bh_off + iq] = m_run[r] + __logf(l_run[r]);
        }
    }
}

}  // namespace

// ======================================================================
// Forward v2 (docs/KERNEL_PLAN_R2.md):
//   * 4 or 8 waves x 32 q rows, v_mfma_f32_32x32x16_bf16 (guide §B 8-warp ladder)
//   * swapped QK^T (St = K·Q^T): the P row for q-row lane&31 is lane-local
//     (32 f32 regs), so softmax is in-register — no p_lds bounce, no
//     __shfl tree (T12: cross-half combine = one permlane32_swap)
//   * swapped PV too (O^T = V^T·P^T): the O accumulator is ALSO per-lane
//     q-row lane&31, so the online-softmax rescale is a scalar broadcast
//     multiply — no cross-lane redistribution of alpha
//   * K and V^T LDS images on 256-B rows with the T2 XOR swizzle
//     (byte ^= (row&15)<<4): the b128 fragment reads are conflict-free
//     (v1's padded rows measured 33-63% LDS bank-conflict cycles)
//   * double-buffered tiles with the T14 split: global loads for tile n+1
//     issue before tile n's QK^T, the LDS write lands after softmax, so HBM
//     latency hides under MFMA; one barrier per tile
__device__ __forceinline__ float u2f(unsigned u) { return __uint_as_float(u); }

namespace {

// Element index into a swizzled [row][128] bf16 image (256-B rows): the
// byte offset within the row is XORed with (row&15)<<4, spreading a b128
// lane group over all 16 slots of the 256-B bank row (T2 / G4).  The XOR
// touches byte-address bits 4-7 only, so 16-B and 4-B alignment survive.
__device__ __forceinline__ int swz128(int row, int elem_col) {
    return row * 128 + ((((elem_col) << 1) ^ ((row & 15) << 4)) >> 1);
}

// Same idea on 128-B rows (64 bf16): 8 slots per row, <=2-way residual.
__device__ __forceinline__ int swz64(int row, int elem_col) {
    return row * 64 + ((((elem_col) << 1) ^ ((row & 7) << 4)) >> 1);
}

template <int RS>
__device__ __forceinline__ int swz_rm(int row, int elem_col) {
    return RS == 64 ? swz64(row, elem_col) : swz128(row, elem_col);
}

// Backward-tile indexers.  Measured split (r2 A/B): for D=128 the 256-B
// swizzled rows beat the padded layout (5797->5474us); for D=64 the padded
// odd strides (72/40) are already conflict-free on the fragment reads and
// swizzled power-of-2 rows REGRESSED (1206->1606us) - keep v1's layout.
template <int D> __device__ __forceinline__ int bwd_rm(int row, int col) {
    return D == 64 ? row * 72 + col : swz128(row, col);
}
template <int D> __device__ __forceinline__ int bwd_tr(int row, int col) {
    return D == 64 ? row * 40 + col : swz64(row, col);
}

// Staging-packet decode for the [4][16]-sub-tiled LDS images: one 16-B
// single-row packet per lane with (col-half e, row&3) in the LOW packet
// bits.  The [4][16] tiles are 128 B (bank-aligned), so a b128 store's
// 8-lane group — which under the naive row-pair mapping varies only the
// column packet — hits the same 8 of 32 banks 4 ways (store bank =
// (addr/4)%32; tile stride ≡ 0).  With (e, rw) in the low 3 lane bits the
// 8 addresses land on banks 8*rw + 4*e + [0..3] = all 32 exactly once,
// while each 16-lane (row) subset of a load instruction still covers one
// contiguous 256-B row slice, so global coalescing is unchanged.
template <int D>
__device__ __forceinline__ void pkt_rc(int p, int& row, int& col) {
    constexpr int DLOG = (D / 16 == 8) ? 3 : 2;
    const int rw = (p >> 1) & 3;
    const int dd = (p >> 3) & (D / 16 - 1);
    row = (p >> (3 + DLOG)) * 4 + rw;
    col = dd * 16 + (p & 1) * 8;
}

// C/D layout of mfma_f32_32x32x16_bf16: col = lane&31, row = (r&3) +
// 8*(r>>2) + 4*(lane>>5), r in [0,16).  A/B fragments: i/j = lane&31,
// k = 8*(lane>>5) + elem (verified by mfma_probe32).
template <int D, int WAVES>
__global__ __launch_bounds__(WAVES * WAVE_SIZE)
void attn_fwd_v2_kernel(const bf16* __restrict__ q, const bf16* __restrict__ k,
                        const bf16* __restrict__ v,
                        const float* __restrict__ slopes, float scale,
                        bf16* __restrict__ o, float* __restrict__ lse,
                        int B, int H, int S, int kv_off, int kv_group,
                        int64_t qb, int64_t qh, int64_t qs,
                        int64_t kb, int64_t kh, int64_t ks,
                        int64_t vb, int64_t vh, int64_t vs,
                        int64_t ob, int64_t oh, int64_t os) {
    constexpr int KVB = 64;                 // kv rows per tile
    constexpr int NT = WAVES * WAVE_SIZE;
    constexpr int ROWS = WAVES * 32;        // q rows per workgroup
    constexpr int DCH = D / 16;             // QK^T k-chunks (K=16 per mfma)
    constexpr int DSUB = D / 32;            // O row subtiles (O^T layout)
    constexpr int NPK = KVB * (D / 8);      // K tile 16-B packets
    constexpr int NPV = KVB * (D / 8);      // V tile single-row packets
    constexpr int KPL = (NPK + NT - 1) / NT;
    constexpr int VPL = (NPV + NT - 1) / NT;
    // V image is [kv/4][d/16][kv%4][16]: each [4 kv][16 d] sub-tile is 128 B
    // contiguous, which is exactly what ds_read_b64_tr_b16 gathers (T10) —
    // the PV A-fragment (V^T) comes out of the hardware transpose read, so
    // no scattered u32 transpose-writes (those were 8-way write conflicts =
    // the 61.6% CONF of the r2 PMC) and half the LDS of the [D][128] image.
    constexpr int VST = (D / 16) * 64;      // elements per 4-kv-row group

    __shared__ __attribute__((aligned(16))) bf16 k_lds[2][KVB * 128];
    __shared__ __attribute__((aligned(16))) bf16 vs_lds[2][KVB * D];

    // XCD-affinity remap (T1): the hardware places linear block id L on XCD
    // L%8, so with qblock fastest-varying the q-blocks sharing one (b,h)'s
    // K/V land on 8 different L2s.  When H*B % 8 == 0, re-deriving (qblock,
    // h, b) with (h,b) fastest pins each (b,h) group to ONE XCD, making its
    // K/V tile L2-resident across q-blocks.  Pure speed, never correctness.
    int qblock = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
    {
        const int ngrp = gridDim.y * gridDim.z;  // H * B
        if ((ngrp & 7) == 0) {
            const int flat = blockIdx.x +
                gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);
            qblock = flat / ngrp;
            const int g = flat % ngrp;
            h = g % gridDim.y;
            b = g / gridDim.y;
        }
    }
    const int tid = threadIdx.x;
    const int wave = tid / WAVE_SIZE;
    const int lane = tid % WAVE_SIZE;
    const int l31 = lane & 31;
    const int hi = lane >> 5;

    const int64_t bh_off = ((int64_t)b * H + h) * S;
    const int hk = h / kv_group;
    const bf16* qp = q + b * qb + h * qh;
    const bf16* kp = k + b * kb + hk * kh;
    const bf16* vp = v + b * vb + hk * vh;
    bf16* op = o + b * ob + h * oh;
    // softmax runs in the exp2 domain (v_exp_f32 is natively exp2): fold
    // log2(e) into scale and slope so no per-element multiply is added
    const float LOG2E = 1.4426950408889634f;
    const float scale2 = scale * LOG2E;
    const float slope2 = slopes[h] * LOG2E;

    const int qr0 = qblock * ROWS + wave * 32;
    const int iq = qr0 + l31;

    frag_ab bQ[DCH];
#pragma unroll
    for (int c = 0; c < DCH; ++c) {
        bQ[c] = *reinterpret_cast<const frag_ab*>(
            qp + (int64_t)iq * qs + c * 16 + 8 * hi);
    }

    f32x16 accO[DSUB];
#pragma unroll
    for (int dsb = 0; dsb < DSUB; ++dsb) {
#pragma unroll
        for (int r = 0; r < 16; ++r) accO[dsb][r] = 0.f;
    }
    float m_run = NEG_INF, l_run = 0.f;

    const bool full_vis = (kv_off <= -S);
    int nkv = full_vis ? (S / KVB)
        : (qblock * ROWS + ROWS - kv_off + KVB - 1) / KVB;
    nkv = min(max(nkv, 0), S / KVB);

    frag_ab kreg[KPL];
    frag_ab vreg[VPL];

    auto stage_load = [&](int nb) {
        const int kvrow0 = nb * KVB;
#pragma unroll
        for (int i = 0; i < KPL; ++i) {
            const int p = tid + i * NT;
            if (p < NPK) {
                const int row = p / (D / 8);
                const int col = (p % (D / 8)) * 8;
                kreg[i] = *reinterpret_cast<const frag_ab*>(
                    kp + (int64_t)(kvrow0 + row) * ks + col);
            }
        }
#pragma unroll
        for (int i = 0; i < VPL; ++i) {
            const int p = tid + i * NT;
            if (p < NPV) {
                int row, col;
                pkt_rc<D>(p, row, col);
                vreg[i] = *reinterpret_cast<const frag_ab*>(
                    vp + (int64_t)(kvrow0 + row) * vs + col);
            }
        }
    };
    auto stage_write = [&](int buf) {
#pragma unroll
        for (int i = 0; i < KPL; ++i) {
            const int p = tid + i * NT;
            if (p < NPK) {
                const int row = p / (D / 8);
                const int col = (p % (D / 8)) * 8;
                *reinterpret_cast<frag_ab*>(&k_lds[buf][swz128(row, col)]) =
                    kreg[i];
            }
        }
#pragma unroll
        for (int i = 0; i < VPL; ++i) {
            const int p = tid + i * NT;
            if (p < NPV) {
                int row, col;
                pkt_rc<D>(p, row, col);
                const int idx = (row >> 2) * VST + (col >> 4) * 64 +
                                (row & 3) * 16 + (col & 15);
                *reinterpret_cast<frag_ab*>(&vs_lds[buf][idx]) = vreg[i];
            }
        }
    };

    if (nkv > 0) {
        stage_load(0);
        stage_write(0);
    }
    __syncthreads();

    for (int nb = 0; nb < nkv; ++nb) {
        const int cur = nb & 1;
        const int kvrow0 = nb * KVB;
        const bool last = (nb + 1 == nkv);
        if (!last) stage_load(nb + 1);   // T14 issue-early

        // a tile entirely above this wave's causal diagonal is skipped
        // (wave-uniform branch; staging stays cooperative)
        const bool active = full_vis || (kvrow0 + kv_off <= qr0 + 31);

        f32x16 st[2];
        frag_ab pfrag[4];
        if (active) {
#pragma unroll
            for (int ns = 0; ns < 2; ++ns) {
#pragma unroll
                for (int r = 0; r < 16; ++r) st[ns][r] = 0.f;
            }
#pragma unroll
            for (int ns = 0; ns < 2; ++ns) {
                __builtin_amdgcn_s_setprio(1);
#pragma unroll
                for (int c = 0; c < DCH; ++c) {
                    frag_ab aK = *reinterpret_cast<const frag_ab*>(
                        &k_lds[cur][swz128(ns * 32 + l31, c * 16 + 8 * hi)]);
                    st[ns] = MFMA_32x32x16(aK, bQ[c], st[ns]);
                }
                __builtin_amdgcn_s_setprio(0);
            }

            // scale + ALiBi + causal mask (exp2 domain); row max in-register
            // as a log-depth tree (a 32-deep serial fmax chain is ~128
            // dependent cycles)
            float mr[32];
#pragma unroll
            for (int ns = 0; ns < 2; ++ns) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int jk = kvrow0 + ns * 32 + (r & 3) + 8 * (r >> 2) +
                                   4 * hi + kv_off;
                    float x = st[ns][r] * scale2 + slope2 * (float)(jk - iq);
                    x = (jk <= iq) ? x : NEG_INF;
                    st[ns][r] = x;
                    mr[ns * 16 + r] = x;
                }
            }
#pragma unroll
            for (int w = 16; w > 0; w >>= 1) {
#pragma unroll
                for (int i = 0; i < w; ++i) mr[i] = fmaxf(mr[i], mr[i + w]);
            }
            float mx = mr[0];
            {   // lanes l and l+32 hold the same q row's two kv halves
                auto sw = __builtin_amdgcn_permlane32_swap(
                    __float_as_uint(mx), __float_as_uint(mx), false, false);
                mx = fmaxf(u2f(sw[0]), u2f(sw[1]));
            }
            const float m_new = fmaxf(m_run, mx);
            // raw v_exp_f32 (arguments are <= 0; results below 2^-126 flush
            // to zero, where exp2f's guarded expansion returned a denormal)
            const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
            m_run = m_new;
            l_run *= alpha;
#pragma unroll
            for (int dsb = 0; dsb < DSUB; ++dsb) {
#pragma unroll
                for (int r = 0; r < 16; ++r) accO[dsb][r] *= alpha;
            }
            float sr[32];
#pragma unroll
            for (int ns = 0; ns < 2; ++ns) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float pv = __builtin_amdgcn_exp2f(st[ns][r] - m_new);
                    st[ns][r] = pv;
                    sr[ns * 16 + r] = pv;
                }
            }
#pragma unroll
            for (int w = 16; w > 0; w >>= 1) {
#pragma unroll
                for (int i = 0; i < w; ++i) sr[i] += sr[i + w];
            }
            float ls = sr[0];
            {
                auto sw = __builtin_amdgcn_permlane32_swap(
                    __float_as_uint(ls), __float_as_uint(ls), false, false);
                ls = u2f(sw[0]) + u2f(sw[1]);
            }
            l_run += ls;

            // pack P into PV B-fragments: lane needs kv = 16*ks + 8*hi + e.
            // Own regs hold kv%8<4 (lower half-wave) / >=4 (upper); one
            // permlane32_swap per word pair completes both fragments (T12).
#pragma unroll
            for (int ns = 0; ns < 2; ++ns) {
#pragma unroll
                for (int hf = 0; hf < 2; ++hf) {
                    union { __bf16 h2[2]; uint32_t u; } wa, wb, wc, wd;
                    wa.h2[0] = (__bf16)st[ns][8 * hf + 0];
                    wa.h2[1] = (__bf16)st[ns][8 * hf + 1];
                    wc.h2[0] = (__bf16)st[ns][8 * hf + 2];
                    wc.h2[1] = (__bf16)st[ns][8 * hf + 3];
                    wb.h2[0] = (__bf16)st[ns][8 * hf + 4];
                    wb.h2[1] = (__bf16)st[ns][8 * hf + 5];
                    wd.h2[0] = (__bf16)st[ns][8 * hf + 6];
                    wd.h2[1] = (__bf16)st[ns][8 * hf + 7];
                    auto s1 = __builtin_amdgcn_permlane32_swap(wa.u, wb.u,
                                                              false, false);
                    auto s2 = __builtin_amdgcn_permlane32_swap(wc.u, wd.u,
                                                              false, false);
                    union { frag_ab f; uint32_t u[4]; } out;
                    out.u[0] = s1[0];
                    out.u[1] = s2[0];
                    out.u[2] = s1[1];
                    out.u[3] = s2[1];
                    pfrag[2 * ns + hf] = out.f;
                }
            }
        }

        if (!last) stage_write(cur ^ 1);  // T14 write-late

        if (active) {
            // O^T += V^T · P^T.  The V^T A-fragment comes from two hardware
            // transpose reads per (dsb, ks): quarter-wave q reads the
            // [4 kv][16 d] sub-tile for d-block 2*dsb+(q&1), kv group
            // 4*ks + 2*hi (+1), and each lane receives its d-column.
            const int lq = lane >> 4;           // quarter-wave index
            const int dblk_off = (lq & 1) * 64; // within-group d-block elems
            const int lel = (lane & 15) * 4;    // lane's element in the tile
#pragma unroll
            for (int dsb = 0; dsb < DSUB; ++dsb) {
                __builtin_amdgcn_s_setprio(1);
#pragma unroll
                for (int ks2 = 0; ks2 < 4; ++ks2) {
                    const int g0 = 4 * ks2 + 2 * hi;
                    const int base = g0 * VST + (2 * dsb) * 64 + dblk_off + lel;
                    union { frag_ab f; bf16x4 h[2]; } av;
                    av.h[0] = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
                        (lds_bf16x4_p)&vs_lds[cur][base]);
                    av.h[1] = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
                        (lds_bf16x4_p)&vs_lds[cur][base + VST]);
                    accO[dsb] = MFMA_32x32x16(av.f, pfrag[ks2], accO[dsb]);
                }
                __builtin_amdgcn_s_setprio(0);
            }
        }
        __syncthreads();
    }

    // epilogue: lane owns q row iq; accO reg r is d = 8*(r>>2)+(r&3)+4*hi
    const float inv_l = (l_run > 0.f) ? 1.0f / l_run : 0.f;
    bf16* orow = op + (int64_t)iq * os;
#pragma unroll
    for (int dsb = 0; dsb < DSUB; ++dsb) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            union { __bf16 h4[4]; uint2 u; } w;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                w.h4[r] = (__bf16)(accO[dsb][4 * g + r] * inv_l);
            }
            *reinterpret_cast<uint2*>(orow + dsb * 32 + 8 * g + 4 * hi) = w.u;
        }
    }
    if (hi == 0) {
        // stats were kept in the exp2 domain; lse is defined in natural log
        lse[bh_off + iq] = 0.6931471805599453f * (m_run + __log2f(l_run));
    }
}

}  // namespace

// ======================================================================
// Backward v1 — two-pass flash2 (no atomics):
//   delta:  delta[m] = rowsum(dO * O)   (shared with the v2 backward)
//   pass A (kv-outer): dK, dV — one workgroup per 64-row kv block,
//                      iterating q blocks >= kv block (causal)
//   pass B (q-outer):  dQ — one workgroup per 64-row q block,
//                      iterating kv blocks <= q block
// Both passes recompute S and P from (q, k, lse): MFMA FLOPs are cheap
// next to re-reading P from HBM.  Each stages BWD_CHUNK rows of the other
// axis per iteration (64-row chunks LDS-capped the kernels to one
// wave/SIMD).
namespace {

constexpr int BWD_CHUNK = 32;

template <int D>
__global__ __launch_bounds__(256)
void attn_bwd_delta_kernel(const bf16* __restrict__ dout,
                           const bf16* __restrict__ o,
                           float* __restrict__ delta, int64_t rows,
                           int H, int S,
                           int64_t db, int64_t dh, int64_t ds_,
                           int64_t ob2, int64_t oh2, int64_t os2) {
    const int64_t row = (int64_t)blockIdx.x * 4 + threadIdx.x / WAVE_SIZE;
    if (row >= rows) return;
    const int lane = threadIdx.x % WAVE_SIZE;
    const int64_t b = row / ((int64_t)H * S);
    const int64_t h = (row / S) % H;
    const int64_t s = row % S;
    const bf16* dr = dout + b * db + h * dh + s * ds_;
    const bf16* orow = o + b * ob2 + h * oh2 + s * os2;
    float acc = 0.f;
    for (int i = lane; i < D; i += WAVE_SIZE) {
        acc += to_float(dr[i]) * to_float(orow[i]);
    }
    acc = wave_reduce_sum(acc);
    if (lane == 0) delta[row] = acc;
}

// pass A: dK(n,:) = scale * sum_m dS(m,n) Q(m,:);  dV(n,:) = sum_m P(m,n) dO(m,:)
template <int D>
__global__ __launch_bounds__(NWAVES * WAVE_SIZE)
void attn_bwd_dkdv_kernel(const bf16* __restrict__ dout,
                          const bf16* __restrict__ q, const bf16* __restrict__ k,
                          const bf16* __restrict__ v,
                          const float* __restrict__ lse,
                          const float* __restrict__ delta,
                          const float* __restrict__ slopes, float scale,
                          bf16* __restrict__ dk, bf16* __restrict__ dv,
                          int B, int H, int S, int kv_off, int kv_group,
                          int64_t gb, int64_t gh, int64_t gs,
                          int64_t qb2, int64_t qh2, int64_t qs2,
                          int64_t kb2, int64_t kh2, int64_t ks2,
                          int64_t vb2, int64_t vh2, int64_t vs2,
                          int64_t wb, int64_t wh, int64_t ws) {
    constexpr int DCH = D / 32;
    constexpr int DSUB = D / 16;
    constexpr int NT = NWAVES * WAVE_SIZE;
    constexpr int QR = BWD_CHUNK;      // q rows staged per iteration
    constexpr int KVROWS = BLOCK_M;    // kv rows per workgroup

    // tile layouts: see bwd_rm / bwd_tr (swizzled power-of-2 rows at D=128,
    // padded odd strides at D=64)
    constexpr int RMS = (D == 64) ? 72 : 128;   // row-major tile stride
    constexpr int TRS = (D == 64) ? 40 : 64;    // transposed tile stride
    __shared__ bf16 do_lds[QR * RMS];
    __shared__ bf16 q_lds[QR * RMS];
    __shared__ bf16 qt_lds[D * TRS];
    __shared__ bf16 dot_lds[D * TRS];
    __shared__ bf16 pt_lds[NWAVES][16 * TRS];   // P^T  (n rows, m cols)
    __shared__ bf16 dst_lds[NWAVES][16 * TRS];  // dS^T (n rows, m cols)
    __shared__ float lse_lds[QR];
    __shared__ float delta_lds[QR];

    const int nb = blockIdx.x;
    const int h = blockIdx.y;
    const int b = blockIdx.z;
    const int tid = threadIdx.x;
    const int wave = tid / WAVE_SIZE;
    const int lane = tid % WAVE_SIZE;
    const int lgrp = lane >> 4, lcol = lane & 15;

    // blockIdx.y is the KV head; the group's q heads accumulate into the
    // same dk/dv (GQA — looping here avoids cross-block write races)
    const int kv0 = nb * KVROWS + wave * 16;  // this wave's 16 kv rows

    // this wave's K and V rows live in registers (A-fragments over d)
    frag_ab aK[DCH], aV[DCH];
    {
        const bf16* krow = k + b * kb2 + h * kh2 + (int64_t)(kv0 + lcol) * ks2;
        const bf16* vrow = v + b * vb2 + h * vh2 + (int64_t)(kv0 + lcol) * vs2;
#pragma unroll
        for (int c = 0; c < DCH; ++c) {
            aK[c] = *reinterpret_cast<const frag_ab*>(krow + c * 32 + 8 * lgrp);
            aV[c] = *reinterpret_cast<const frag_ab*>(vrow + c * 32 + 8 * lgrp);
        }
    }

    frag_cd accDK[DSUB], accDV[DSUB];
#pragma unroll
    for (int s = 0; s < DSUB; ++s) {
        accDK[s] = frag_cd{0.f, 0.f, 0.f, 0.f};
        accDV[s] = frag_cd{0.f, 0.f, 0.f, 0.f};
    }

    for (int gq = 0; gq < kv_group; ++gq) {
    const int hq = h * kv_group + gq;
    const int64_t bh_off = ((int64_t)b * H + hq) * S;  // lse/delta layout
    const bf16* qp = q + b * qb2 + hq * qh2;
    const bf16* dop = dout + b * gb + hq * gh;
    const float slope = slopes[hq];

    const float LOG2E = 1.4426950408889634f;
    const float scale2 = scale * LOG2E;
    const float slope2 = slope * LOG2E;
    // first q row that sees this block's first kv row, rounded down to a
    // chunk boundary: chunks stay aligned, so the last one ends at S for a
    // kv_off that is no multiple of QR too (the rows below the diagonal that
    // the rounding adds are masked elementwise)
    const int q_start = (kv_off <= -S) ? 0
        : max(0, nb * KVROWS + kv_off) & ~(QR - 1);
    for (int q0 = q_start; q0 < S; q0 += QR) {
        __syncthreads();
        {   // stage Q and dO, row-major + transposed, plus lse/delta
            constexpr int PACKETS = (QR / 2) * (D / 8);
            for (int p = tid; p < PACKETS; p += NT) {
                const int row = (p / (D / 8)) * 2;
                const int col = (p % (D / 8)) * 8;
                frag_ab pq0 = *reinterpret_cast<const frag_ab*>(
                    qp + (int64_t)(q0 + row) * qs2 + col);
                frag_ab pq1 = *reinterpret_cast<const frag_ab*>(
                    qp + (int64_t)(q0 + row + 1) * qs2 + col);
                frag_ab pd0 = *reinterpret_cast<const frag_ab*>(
                    dop + (int64_t)(q0 + row) * gs + col);
                frag_ab pd1 = *reinterpret_cast<const frag_ab*>(
                    dop + (int64_t)(q0 + row + 1) * gs + col);
                *reinterpret_cast<frag_ab*>(&q_lds[bwd_rm<D>(row, col)]) = pq0;
                *reinterpret_cast<frag_ab*>(&q_lds[bwd_rm<D>(row + 1, col)]) = pq1;
                *reinterpret_cast<frag_ab*>(&do_lds[bwd_rm<D>(row, col)]) = pd0;
                *reinterpret_cast<frag_ab*>(&do_lds[bwd_rm<D>(row + 1, col)]) = pd1;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    union { __bf16 h[2]; uint32_t u; } a, b2;
                    a.h[0] = pq0[j]; a.h[1] = pq1[j];
                    b2.h[0] = pd0[j]; b2.h[1] = pd1[j];
                    *reinterpret_cast<uint32_t*>(&qt_lds[bwd_tr<D>(col + j, row)]) = a.u;
                    *reinterpret_cast<uint32_t*>(&dot_lds[bwd_tr<D>(col + j, row)]) = b2.u;
                }
            }
            for (int i = tid; i < QR; i += NT) {
                lse_lds[i] = lse[bh_off + q0 + i] * LOG2E;
                delta_lds[i] = delta[bh_off + q0 + i];
            }
        }
        __syncthreads();

        // build P^T and dS^T for ALL QR q columns of this chunk
#pragma unroll
        for (int ms = 0; ms < QR / 16; ++ms) {
            frag_cd st = frag_cd{0.f, 0.f, 0.f, 0.f};
            frag_cd dpt = frag_cd{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int c = 0; c < DCH; ++c) {
                frag_ab bQ = *reinterpret_cast<const frag_ab*>(
                    &q_lds[bwd_rm<D>(ms * 16 + lcol, c * 32 + 8 * lgrp)]);
                st = MFMA_16x16x32(aK[c], bQ, st);          // S^T = K·Q^T
                frag_ab bDO = *reinterpret_cast<const frag_ab*>(
                    &do_lds[bwd_rm<D>(ms * 16 + lcol, c * 32 + 8 * lgrp)]);
                dpt = MFMA_16x16x32(aV[c], bDO, dpt);       // dP^T = V·dO^T
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int n_glob = kv0 + 4 * lgrp + r + kv_off;
                const int m_loc = ms * 16 + lcol;
                const int m_glob = q0 + m_loc;
                float z = st[r] * scale2 + slope2 * (float)(n_glob - m_glob);
                float p = (n_glob <= m_glob) ? exp2f(z - lse_lds[m_loc]) : 0.f;
                float ds = p * (dpt[r] - delta_lds[m_loc]) * scale;
                pt_lds[wave][bwd_tr<D>(4 * lgrp + r, m_loc)] = (bf16)p;
                dst_lds[wave][bwd_tr<D>(4 * lgrp + r, m_loc)] = (bf16)ds;
            }
        }
        __builtin_amdgcn_s_waitcnt(0);  // own-wave LDS writes visible

        // dV += P^T·dO and dK += dS^T·Q over the QR q rows
#pragma unroll
        for (int kc = 0; kc < QR / 32; ++kc) {
            frag_ab aPT = *reinterpret_cast<const frag_ab*>(
                &pt_lds[wave][bwd_tr<D>(lcol, kc * 32 + 8 * lgrp)]);
            frag_ab aDST = *reinterpret_cast<const frag_ab*>(
                &dst_lds[wave][bwd_tr<D>(lcol, kc * 32 + 8 * lgrp)]);
#pragma unroll
            for (int ds = 0; ds < DSUB; ++ds) {
                frag_ab bDOT = *reinterpret_cast<const frag_ab*>(
                    &dot_lds[bwd_tr<D>(ds * 16 + lcol, kc * 32 + 8 * lgrp)]);
                accDV[ds] = MFMA_16x16x32(aPT, bDOT, accDV[ds]);
                frag_ab bQT = *reinterpret_cast<const frag_ab*>(
                    &qt_lds[bwd_tr<D>(ds * 16 + lcol, kc * 32 + 8 * lgrp)]);
                accDK[ds] = MFMA_16x16x32(aDST, bQT, accDK[ds]);
            }
        }
    }

    }  // gq (GQA group loop)

    // epilogue: C row = this wave's kv row (4*lgrp+reg), col = d
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int n_glob = kv0 + 4 * lgrp + r;
        bf16* dkrow = dk + b * wb + h * wh + (int64_t)n_glob * ws;
        bf16* dvrow = dv + b * wb + h * wh + (int64_t)n_glob * ws;
#pragma unroll
        for (int ds = 0; ds < DSUB; ++ds) {
            dkrow[ds * 16 + lcol] = (bf16)accDK[ds][r];
            dvrow[ds * 16 + lcol] = (bf16)accDV[ds][r];
        }
    }
}

// pass B: dQ(m,:) = scale * sum_n dS(m,n) K(n,:)
template <int D>
__global__ __launch_bounds__(NWAVES * WAVE_SIZE)
void attn_bwd_dq_kernel(const bf16* __restrict__ dout,
                        const bf16* __restrict__ q, const bf16* __restrict__ k,
                        const bf16* __restrict__ v,
                        const float* __restrict__ lse,
                        const float* __restrict__ delta,
                        const float* __restrict__ slopes, float scale,
                        bf16* __restrict__ dq,
                        int B, int H, int S, int kv_off, int kv_group,
                        int64_t gb, int64_t gh, int64_t gs,
                        int64_t qb2, int64_t qh2, int64_t qs2,
                        int64_t kb2, int64_t kh2, int64_t ks2,
                        int64_t vb2, int64_t vh2, int64_t vs2,
                        int64_t wb, int64_t wh, int64_t ws) {
    constexpr int DCH = D / 32;
    constexpr int DSUB = D / 16;
    constexpr int NT = NWAVES * WAVE_SIZE;
    constexpr int KVR = BWD_CHUNK;         // kv rows staged per iteration
    constexpr int QROWS = BLOCK_M;         // q rows per workgroup

    // same tile strides as dkdv
    constexpr int RMS = (D == 64) ? 72 : 128;
    constexpr int TRS = (D == 64) ? 40 : 64;
    __shared__ bf16 k_lds[KVR * RMS];       // row-major K (QK^T B-frags)
    __shared__ bf16 v_lds[KVR * RMS];       // row-major V (dP B-frags)
    __shared__ bf16 kt_lds[D * TRS];        // transposed K (dQ B-frags)
    __shared__ bf16 ds_lds[NWAVES][16 * TRS];  // dS (m rows, n cols)

    const int qb = blockIdx.x;
    const int h = blockIdx.y;
    const int b = blockIdx.z;
    const int tid = threadIdx.x;
    const int wave = tid / WAVE_SIZE;
    const int lane = tid % WAVE_SIZE;
    const int lgrp = lane >> 4, lcol = lane & 15;

    const int64_t bh_off = ((int64_t)b * H + h) * S;  // lse/delta layout
    const int hk = h / kv_group;  // GQA
    const bf16* kp = k + b * kb2 + hk * kh2;
    const bf16* vp = v + b * vb2 + hk * vh2;
    const float slope = slopes[h];

    const int qrow0 = qb * QROWS + wave * 16;

    // Q and dO rows of this wave in registers; lse/delta per owned row
    frag_ab aQ[DCH], aDO[DCH];
    {
        const bf16* qrow = q + b * qb2 + h * qh2 + (int64_t)(qrow0 + lcol) * qs2;
        const bf16* dorow = dout + b * gb + h * gh + (int64_t)(qrow0 + lcol) * gs;
#pragma unroll
        for (int c = 0; c < DCH; ++c) {
            aQ[c] = *reinterpret_cast<const frag_ab*>(qrow + c * 32 + 8 * lgrp);
            aDO[c] = *reinterpret_cast<const frag_ab*>(dorow + c * 32 + 8 * lgrp);
        }
    }
    const float LOG2E = 1.4426950408889634f;
    const float scale2 = scale * LOG2E;
    const float slope2 = slope * LOG2E;
    float lse_r[4], delta_r[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int iq = qrow0 + 4 * lgrp + r;
        lse_r[r] = lse[bh_off + iq] * LOG2E;
        delta_r[r] = delta[bh_off + iq];
    }

    frag_cd accDQ[DSUB];
#pragma unroll
    for (int s = 0; s < DSUB; ++s) accDQ[s] = frag_cd{0.f, 0.f, 0.f, 0.f};

    const int kv_end = (kv_off <= -S) ? S
        : min((int64_t)S, (int64_t)qb * QROWS + QROWS - kv_off);  // causal bound
    for (int kv0 = 0; kv0 < kv_end; kv0 += KVR) {
        __syncthreads();
        {   // stage K (row-major + transposed) and V (row-major)
            constexpr int PACKETS = (KVR / 2) * (D / 8);
            for (int p = tid; p < PACKETS; p += NT) {
                const int row = (p / (D / 8)) * 2;
                const int col = (p % (D / 8)) * 8;
                frag_ab pk0 = *reinterpret_cast<const frag_ab*>(
                    kp + (int64_t)(kv0 + row) * ks2 + col);
                frag_ab pk1 = *reinterpret_cast<const frag_ab*>(
                    kp + (int64_t)(kv0 + row + 1) * ks2 + col);
                frag_ab pv0 = *reinterpret_cast<const frag_ab*>(
                    vp + (int64_t)(kv0 + row) * vs2 + col);
                frag_ab pv1 = *reinterpret_cast<const frag_ab*>(
                    vp + (int64_t)(kv0 + row + 1) * vs2 + col);
                *reinterpret_cast<frag_ab*>(&k_lds[bwd_rm<D>(row, col)]) = pk0;
                *reinterpret_cast<frag_ab*>(&k_lds[bwd_rm<D>(row + 1, col)]) = pk1;
                *reinterpret_cast<frag_ab*>(&v_lds[bwd_rm<D>(row, col)]) = pv0;
                *reinterpret_cast<frag_ab*>(&v_lds[bwd_rm<D>(row + 1, col)]) = pv1;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    union { __bf16 h[2]; uint32_t u; } a;
                    a.h[0] = pk0[j]; a.h[1] = pk1[j];
                    *reinterpret_cast<uint32_t*>(&kt_lds[bwd_tr<D>(col + j, row)]) = a.u;
                }
            }
        }
        __syncthreads();

        // dS for all KVR kv cols of this chunk
#pragma unroll
        for (int ns = 0; ns < KVR / 16; ++ns) {
            frag_cd sacc = frag_cd{0.f, 0.f, 0.f, 0.f};
            frag_cd dpacc = frag_cd{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int c = 0; c < DCH; ++c) {
                frag_ab bK = *reinterpret_cast<const frag_ab*>(
                    &k_lds[bwd_rm<D>(ns * 16 + lcol, c * 32 + 8 * lgrp)]);
                sacc = MFMA_16x16x32(aQ[c], bK, sacc);      // S = Q·K^T
                frag_ab bV = *reinterpret_cast<const frag_ab*>(
                    &v_lds[bwd_rm<D>(ns * 16 + lcol, c * 32 + 8 * lgrp)]);
                dpacc = MFMA_16x16x32(aDO[c], bV, dpacc);   // dP = dO·V^T
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int iq = qrow0 + 4 * lgrp + r;
                const int jk = kv0 + ns * 16 + lcol + kv_off;
                float z = sacc[r] * scale2 + slope2 * (float)(jk - iq);
                float p = (jk <= iq) ? exp2f(z - lse_r[r]) : 0.f;
                float ds = p * (dpacc[r] - delta_r[r]) * scale;
                // store transposed to [m][n] so the dQ A-frag read is linear
                ds_lds[wave][bwd_tr<D>(4 * lgrp + r, ns * 16 + lcol)] = (bf16)ds;
            }
        }
        __builtin_amdgcn_s_waitcnt(0);

        // dQ += dS·K over the KVR kv rows
#pragma unroll
        for (int kc = 0; kc < KVR / 32; ++kc) {
            frag_ab aDS = *reinterpret_cast<const frag_ab*>(
                &ds_lds[wave][bwd_tr<D>(lcol, kc * 32 + 8 * lgrp)]);
#pragma unroll
            for (int ds = 0; ds < DSUB; ++ds) {
                frag_ab bKT = *reinterpret_cast<const frag_ab*>(
                    &kt_lds[bwd_tr<D>(ds * 16 + lcol, kc * 32 + 8 * lgrp)]);
                accDQ[ds] = MFMA_16x16x32(aDS, bKT, accDQ[ds]);
            }
        }
    }

#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int iq = qrow0 + 4 * lgrp + r;
        bf16* dqrow = dq + b * wb + h * wh + (int64_t)iq * ws;
#pragma unroll
        for (int ds = 0; ds < DSUB; ++ds) {
            dqrow[ds * 16 + lcol] = (bf16)accDQ[ds][r];
        }
    }
}

}  // namespace

// ======================================================================
// Backward v2 — same ladder as the forward (32x32 MFMA, lane-local
// layouts, swizzled/subtiled LDS, exp2 domain).  Two kernels:
//   dq_v2   (q-outer):  wave owns 32 q rows; K/V tiles staged; St^T and
//           dP^T have q on the lane axis (lse/delta are per-lane scalars),
//           dS packs into B-fragments and dQ^T accumulates lane-locally.
//   dkdv_v2 (kv-outer): wave owns 32 kv rows (K/V B-fragments live in
//           registers); Q/dO tiles staged in the sub-tiled image, which
//           serves BOTH the row-major A-fragments (St, dP) and the
//           hardware-transpose reads (dV^T = dO^T·P, dK^T = Q^T·dS).
// The sub-tiled image is [rows/4][d/16][4][16] with the d-block position
// XORed by the row-group (tiles stay 128-B contiguous for tr16 while the
// row-major reads spread across banks).
namespace {

// The D=128 kernels sit at the register cap, and a second (mask-free) copy
// of the sub-tile body makes them spill: they keep one body that applies the
// mask as a select on every sub-tile (a no-op for fully visible launches).
template <int D> constexpr bool peel_unmasked = (D == 64);

// a*b + c*d with BOTH products rounded before the add. The dkdv kernels have
// always formed the exponent this way; a contracted fma would move its
// roundings, and with them bits of P, dS and every gradient.
__device__ __forceinline__ float mul2_add(float a, float b, float c, float d) {
#pragma clang fp contract(off)
    return a * b + c * d;
}

// two floats -> one packed bf16 pair (round-to-nearest-even): a vector
// conversion, so that it compiles to ONE v_cvt_pk_bf16_f32 (converting the
// halves one by one costs two of them plus a shift and an or per pair)
__device__ __forceinline__ uint32_t pack_bf16x2(float lo, float hi) {
    using f32x2 = __attribute__((ext_vector_type(2))) float;
    using bf16x2 = __attribute__((ext_vector_type(2))) __bf16;
    const f32x2 f = {lo, hi};
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(f, bf16x2));
}

// Half hf of a 32x32 C fragment (8 registers) as a B-fragment with the C
// row axis as k: each lane holds rows 8g + 4*hi + 0..3 and needs 8
// consecutive ones, so the half-waves exchange word pairs.
__device__ __forceinline__ frag_ab c_to_bfrag(const f32x16& x, int hf) {
    const uint32_t wa = pack_bf16x2(x[8 * hf + 0], x[8 * hf + 1]);
    const uint32_t wc = pack_bf16x2(x[8 * hf + 2], x[8 * hf + 3]);
    const uint32_t wb = pack_bf16x2(x[8 * hf + 4], x[8 * hf + 5]);
    const uint32_t wd = pack_bf16x2(x[8 * hf + 6], x[8 * hf + 7]);
    auto s1 = __builtin_amdgcn_permlane32_swap(wa, wb, false, false);
    auto s2 = __builtin_amdgcn_permlane32_swap(wc, wd, false, false);
    union { frag_ab f; uint32_t u[4]; } out;
    out.u[0] = s1[0];
    out.u[1] = s2[0];
    out.u[2] = s1[1];
    out.u[3] = s2[1];
    return out.f;
}

// element index into a sub-tiled [R][D] image; DBLK = D/16
template <int D>
__device__ __forceinline__ int sub_idx(int row, int elem_col) {
    constexpr int DBLK = D / 16;
    const int g = row >> 2;
    const int dblk = (elem_col >> 4) ^ (g & (DBLK - 1));
    return g * (DBLK * 64) + dblk * 64 + (row & 3) * 16 + (elem_col & 15);
}

// byte-base of the [4][16] tr16 tile for (row group g, logical d-block)
template <int D>
__device__ __forceinline__ int sub_tile_base(int g, int dblk_log) {
    constexpr int DBLK = D / 16;
    return g * (DBLK * 64) + (dblk_log ^ (g & (DBLK - 1))) * 64;
}

template <int D, int WAVES>
__global__ __launch_bounds__(WAVES * WAVE_SIZE)
void attn_bwd_dq_v2_kernel(const bf16* __restrict__ dout,
                           const bf16* __restrict__ q, const bf16* __restrict__ k,
                           const bf16* __restrict__ v,
                           const float* __restrict__ lse,
                           const float* __restrict__ delta,
                           const float* __restrict__ slopes, float scale,
                           bf16* __restrict__ dq,
                           int B, int H, int S, int kv_off, int kv_group,
                           int64_t gb, int64_t gh, int64_t gs,
                           int64_t qb2, int64_t qh2, int64_t qs2,
                           int64_t kb2, int64_t kh2, int64_t ks2,
                           int64_t vb2, int64_t vh2, int64_t vs2,
                           int64_t wb, int64_t wh, int64_t ws) {
    constexpr int KVB = 64;
    constexpr int NT = WAVES * WAVE_SIZE;
    constexpr int ROWS = WAVES * 32;
    constexpr int DCH = D / 16;
    constexpr int DSUB = D / 32;
    constexpr bool PEEL = peel_unmasked<D>;
    constexpr int VST = (D / 16) * 64;
    constexpr int NPK = KVB * (D / 8);          // K single-row packets
    constexpr int KPL = (NPK + NT - 1) / NT;
    constexpr int NP = (KVB / 2) * (D / 8);     // V row-pair packets
    constexpr int PPL = (NP + NT - 1) / NT;

    __shared__ __attribute__((aligned(16))) bf16 ks_lds[2][KVB * D];
    __shared__ __attribute__((aligned(16))) bf16 v_lds[2][KVB * 128];

    const int qblock = blockIdx.x;
    const int h = blockIdx.y;
    const int b = blockIdx.z;
    const int tid = threadIdx.x;
    const int wave = tid / WAVE_SIZE;
    const int lane = tid % WAVE_SIZE;
    const int l31 = lane & 31;
    const int hi = lane >> 5;
    const int lq = lane >> 4;

    const int64_t bh_off = ((int64_t)b * H + h) * S;
    const int hk = h / kv_group;
    const bf16* kp = k + b * kb2 + hk * kh2;
    const bf16* vp = v + b * vb2 + hk * vh2;
    const float LOG2E = 1.4426950408889634f;
    const float scale2 = scale * LOG2E;
    const float slope2 = slopes[h] * LOG2E;

    const int qr0 = qblock * ROWS + wave * 32;
    const int iq = qr0 + l31;
    // same value, but known wave-uniform to the compiler: the tile
    // classification below then branches on scalars, not on EXEC
    const int qr0_u = __builtin_amdgcn_readfirstlane(qr0);

    frag_ab bQ[DCH], bDO[DCH];
    {
        const bf16* qrow = q + b * qb2 + h * qh2 + (int64_t)iq * qs2;
        const bf16* dorow = dout + b * gb + h * gh + (int64_t)iq * gs;
#pragma unroll
        for (int c = 0; c < DCH; ++c) {
            bQ[c] = *reinterpret_cast<const frag_ab*>(qrow + c * 16 + 8 * hi);
            bDO[c] = *reinterpret_cast<const frag_ab*>(dorow + c * 16 + 8 * hi);
        }
    }
    const float lse2 = lse[bh_off + iq] * LOG2E;
    const float dlt = delta[bh_off + iq];

    f32x16 accDQ[DSUB];
#pragma unroll
    for (int dsb = 0; dsb < DSUB; ++dsb) {
#pragma unroll
        for (int r = 0; r < 16; ++r) accDQ[dsb][r] = 0.f;
    }

    const bool full_vis = (kv_off <= -S);
    const int kv_end = full_vis ? S
        : min(S, qblock * ROWS + ROWS - kv_off);
    const int nkv = max(0, (kv_end + KVB - 1) / KVB);

    frag_ab kreg[KPL], vreg[PPL][2];
    auto stage_load = [&](int nb) {
        const int kvrow0 = nb * KVB;
#pragma unroll
        for (int i = 0; i < KPL; ++i) {
            const int p = tid + i * NT;
            if (p < NPK) {
                int row, col;
                pkt_rc<D>(p, row, col);
                kreg[i] = *reinterpret_cast<const frag_ab*>(
                    kp + (int64_t)(kvrow0 + row) * ks2 + col);
            }
        }
#pragma unroll
        for (int i = 0; i < PPL; ++i) {
            const int p = tid + i * NT;
            if (p < NP) {
                const int row = (p / (D / 8)) * 2;
                const int col = (p % (D / 8)) * 8;
                vreg[i][0] = *reinterpret_cast<const frag_ab*>(
                    vp + (int64_t)(kvrow0 + row) * vs2 + col);
                vreg[i][1] = *reinterpret_cast<const frag_ab*>(
                    vp + (int64_t)(kvrow0 + row + 1) * vs2 + col);
            }
        }
    };
    auto stage_write = [&](int buf) {
#pragma unroll
        for (int i = 0; i < KPL; ++i) {
            const int p = tid + i * NT;
            if (p < NPK) {
                int row, col;
                pkt_rc<D>(p, row, col);
                *reinterpret_cast<frag_ab*>(
                    &ks_lds[buf][sub_idx<D>(row, col)]) = kreg[i];
            }
        }
#pragma unroll
        for (int i = 0; i < PPL; ++i) {
            const int p = tid + i * NT;
            if (p < NP) {
                const int row = (p / (D / 8)) * 2;
                const int col = (p % (D / 8)) * 8;
#pragma unroll
                for (int rr = 0; rr < 2; ++rr) {
                    *reinterpret_cast<frag_ab*>(
                        &v_lds[buf][swz128(row + rr, col)]) = vreg[i][rr];
                }
            }
        }
    };

    constexpr bool EARLY_LOAD = true;
    if (nkv > 0) {
        stage_load(0);
        stage_write(0);
    }
    __syncthreads();

    for (int nb = 0; nb < nkv; ++nb) {
        const int cur = nb & 1;
        const int kvrow0 = nb * KVB;
        const bool last = (nb + 1 == nkv);
        if (EARLY_LOAD && !last) stage_load(nb + 1);

        const bool active = full_vis || (kvrow0 + kv_off <= qr0_u + 31);
        if (active) {
            // D=128 must NOT unroll (doubled live f32x16 pairs spill);
            // D=64 has register headroom and full unroll measured faster.
            // MASKED is a compile-time tag: sub-tiles wholly at or below the
            // wave's diagonal run the body without any mask instruction.
            auto ns_body = [&](int ns, auto masked_t) {
                constexpr bool MASKED = decltype(masked_t)::value;
                frag_ab dsfrag[2];
                f32x16 st, dp;
#pragma unroll
                for (int r = 0; r < 16; ++r) { st[r] = 0.f; dp[r] = 0.f; }
                __builtin_amdgcn_s_setprio(1);
#pragma unroll
                for (int c = 0; c < DCH; ++c) {
                    // St^T = K·Q^T: A = K row-major from the sub-tiled image
                    frag_ab aK = *reinterpret_cast<const frag_ab*>(
                        &ks_lds[cur][sub_idx<D>(ns * 32 + l31, c * 16 + 8 * hi)]);
                    st = MFMA_32x32x16(aK, bQ[c], st);
                    frag_ab aV = *reinterpret_cast<const frag_ab*>(
                        &v_lds[cur][swz128(ns * 32 + l31, c * 16 + 8 * hi)]);
                    dp = MFMA_32x32x16(aV, bDO[c], dp);  // dP^T = V·dO^T
                }
                __builtin_amdgcn_s_setprio(0);
                // softmax/dS phase. Register r is kv row jk = iq + dj + roff(r)
                // with roff(r) = 8*(r>>2) + (r&3). Every value is rounded
                // exactly where it always was (st*scale2, then one fma with
                // the bias, then -lse2; dS scaled per element), so results
                // are bitwise what the branchy form gave; only the work
                // around them is gone. The position difference goes to float
                // once per sub-tile: dj and roff are small integers, so
                // fdj + roff is exact. The exponent is <= ~0 for live
                // elements (lse is the row's log-sum), so the raw v_exp_f32
                // serves: results below 2^-126 flush to zero and vanish in
                // the bf16 rounding. Masked elements are selected away AFTER
                // the exp (it may be +inf there), never multiplied.
                const int dj = kvrow0 + ns * 32 + 4 * hi + kv_off - iq;
                const float fdj = (float)dj;
                const bool all_live = !PEEL && full_vis;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int roff = (r & 3) + 8 * (r >> 2);
                    const float z2 = fmaf(slope2, fdj + (float)roff,
                                          st[r] * scale2);
                    float p = __builtin_amdgcn_exp2f(z2 - lse2);
                    if (MASKED) p = (all_live || dj + roff <= 0) ? p : 0.f;
                    st[r] = p * (dp[r] - dlt) * scale;  // dS^T
                }
                // pack dS^T into B-fragments (k = kv), as in the forward
#pragma unroll
                for (int hf = 0; hf < 2; ++hf) dsfrag[hf] = c_to_bfrag(st, hf);
                // dQ^T += K^T·dS^T for this ns's two kv chunks (keeps the
                // fragment set at 2 so D=128 stays under the VGPR cap)
#pragma unroll
                for (int dsb = 0; dsb < DSUB; ++dsb) {
                    __builtin_amdgcn_s_setprio(1);
#pragma unroll
                    for (int ksq = 0; ksq < 2; ++ksq) {
                        const int g0 = 8 * ns + 4 * ksq + 2 * hi;
                        const int dblk = 2 * dsb + (lq & 1);
                        union { frag_ab f; bf16x4 h[2]; } akt;
                        akt.h[0] = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
                            (lds_bf16x4_p)&ks_lds[cur][
                                sub_tile_base<D>(g0, dblk) + (lane & 15) * 4]);
                        akt.h[1] = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
                            (lds_bf16x4_p)&ks_lds[cur][
                                sub_tile_base<D>(g0 + 1, dblk) + (lane & 15) * 4]);
                        accDQ[dsb] = MFMA_32x32x16(akt.f, dsfrag[ksq],
                                                   accDQ[dsb]);
                    }
                    __builtin_amdgcn_s_setprio(0);
                }
            };
            // wave-uniform classification of one 32x32 sub-tile: no kv row
            // of it lies above the wave's first q row
            auto ns_run = [&](int ns) {
                if (PEEL &&
                    (full_vis || kvrow0 + ns * 32 + 31 + kv_off <= qr0_u))
                    ns_body(ns, std::false_type{});
                else
                    ns_body(ns, std::true_type{});
            };
            if (D == 128) {
#pragma unroll 1
                for (int ns = 0; ns < 2; ++ns) ns_run(ns);
            } else {
                ns_run(0);
                ns_run(1);
            }
        }
        if (!last) {
            if (!EARLY_LOAD) stage_load(nb + 1);
            stage_write(cur ^ 1);
        }
        __syncthreads();
    }

    // epilogue: dq row iq; reg r is d = 8*(r>>2)+(r&3)+4*hi  (dS already
    // carries the softmax-scale factor)
    bf16* dqrow = dq + b * wb + h * wh + (int64_t)iq * ws;
#pragma unroll
    for (int dsb = 0; dsb < DSUB; ++dsb) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            union { __bf16 h4[4]; uint2 u; } w;
#pragma unroll
            for (int r = 0; r < 4; ++r) w.h4[r] = (__bf16)accDQ[dsb][4 * g + r];
            *reinterpret_cast<uint2*>(dqrow + dsb * 32 + 8 * g + 4 * hi) = w.u;
        }
    }
}

// DKPART: -1 = accumulate dK over all of D; 0/1 = only that d-half (the
// dk pass at D=128 exceeds the 8-wave register cap with a full-width
// accumulator — two half-width launches recompute St/dP but run at
// 2 waves/SIMD instead of the 4-wave build's 1)
template <int D, int WAVES, bool DO_DK, bool DO_DV, int DKPART = -1>
__global__ __launch_bounds__(WAVES * WAVE_SIZE)
void attn_bwd_dkdv_v2_kernel(const bf16* __restrict__ dout,
                             const bf16* __restrict__ q, const bf16* __restrict__ k,
                             const bf16* __restrict__ v,
                             const float* __restrict__ lse,
                             const float* __restrict__ delta,
                             const float* __restrict__ slopes, float scale,
                             bf16* __restrict__ dk, bf16* __restrict__ dv,
                             int B, int H, int S, int kv_off, int kv_group,
                             int64_t gb, int64_t gh, int64_t gs,
                             int64_t qb2, int64_t qh2, int64_t qs2,
                             int64_t kb2, int64_t kh2, int64_t ks2,
                             int64_t vb2, int64_t vh2, int64_t vs2,
                             int64_t wb, int64_t wh, int64_t ws) {
    constexpr int QT = 64;                   // q rows staged per tile
    constexpr int NT = WAVES * WAVE_SIZE;
    constexpr int ROWS = WAVES * 32;         // kv rows per workgroup
    constexpr int DCH = D / 16;
    constexpr int DSUB = D / 32;
    constexpr int NP = QT * (D / 8);         // single-row staging packets
    constexpr bool PEEL = peel_unmasked<D>;
    constexpr int PPL = (NP + NT - 1) / NT;

    __shared__ __attribute__((aligned(16))) bf16 qs_lds[2][QT * D];
    __shared__ __attribute__((aligned(16))) bf16 dos_lds[2][QT * D];
    // row statistics, 16-B aligned for the b128 reads of the softmax phase
    __shared__ __attribute__((aligned(16))) float lse_lds[2][QT];
    __shared__ __attribute__((aligned(16))) float dlt_lds[2][QT];

    const int nb = blockIdx.x;
    const int h = blockIdx.y;   // KV head
    const int b = blockIdx.z;
    const int tid = threadIdx.x;
    const int wave = tid / WAVE_SIZE;
    const int lane = tid % WAVE_SIZE;
    const int l31 = lane & 31;
    const int hi = lane >> 5;
    const int lq = lane >> 4;

    const int kv0w = nb * ROWS + wave * 32;  // wave's kv rows
    const int n_glob = kv0w + l31;
    // same value, but known wave-uniform to the compiler (scalar branches
    // for the tile skip and the masked/unmasked classification)
    const int kv0w_u = __builtin_amdgcn_readfirstlane(kv0w);
    const float LOG2E = 1.4426950408889634f;
    const float scale2 = scale * LOG2E;

    constexpr int DK0 = (DKPART < 0) ? 0 : DKPART * (DSUB / 2);
    constexpr int NDSB = (DKPART < 0) ? DSUB : DSUB / 2;
    frag_ab bK[DCH], bV[DO_DK ? DCH : 1];
    {
        const bf16* krow = k + b * kb2 + h * kh2 + (int64_t)n_glob * ks2;
        const bf16* vrow = v + b * vb2 + h * vh2 + (int64_t)n_glob * vs2;
#pragma unroll
        for (int c = 0; c < DCH; ++c) {
            bK[c] = *reinterpret_cast<const frag_ab*>(krow + c * 16 + 8 * hi);
            if (DO_DK)
                bV[c] = *reinterpret_cast<const frag_ab*>(vrow + c * 16 + 8 * hi);
        }
    }
    f32x16 accDK[DO_DK ? NDSB : 1], accDV[DO_DV ? DSUB : 1];
#pragma unroll
    for (int dsb = 0; dsb < DSUB; ++dsb) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            if (DO_DK && dsb < NDSB) accDK[dsb][r] = 0.f;
            if (DO_DV) accDV[dsb][r] = 0.f;
        }
    }

    const bool full_vis = (kv_off <= -S);
    const int q_first = full_vis ? 0
        : max(0, (nb * ROWS + kv_off) & ~(QT - 1));

    for (int gq = 0; gq < kv_group; ++gq) {
        const int hq = h * kv_group + gq;
        const int64_t bh_off = ((int64_t)b * H + hq) * S;
        const bf16* qp = q + b * qb2 + hq * qh2;
        const bf16* dop = dout + b * gb + hq * gh;
        const float slope2 = slopes[hq] * LOG2E;

        frag_ab qreg[PPL], doreg[PPL];
        auto stage_load = [&](int q0) {
#pragma unroll
            for (int i = 0; i < PPL; ++i) {
                const int p = tid + i * NT;
                if (p < NP) {
                    int row, col;
                    pkt_rc<D>(p, row, col);
                    qreg[i] = *reinterpret_cast<const frag_ab*>(
                        qp + (int64_t)(q0 + row) * qs2 + col);
                    doreg[i] = *reinterpret_cast<const frag_ab*>(
                        dop + (int64_t)(q0 + row) * gs + col);
                }
            }
        };
        auto stage_write = [&](int buf, int q0) {
#pragma unroll
            for (int i = 0; i < PPL; ++i) {
                const int p = tid + i * NT;
                if (p < NP) {
                    int row, col;
                    pkt_rc<D>(p, row, col);
                    *reinterpret_cast<frag_ab*>(
                        &qs_lds[buf][sub_idx<D>(row, col)]) = qreg[i];
                    *reinterpret_cast<frag_ab*>(
                        &dos_lds[buf][sub_idx<D>(row, col)]) = doreg[i];
                }
            }
            for (int i = tid; i < QT; i += NT) {
                lse_lds[buf][i] = lse[bh_off + q0 + i] * LOG2E;
                dlt_lds[buf][i] = delta[bh_off + q0 + i];
            }
        };

        // dk-only at D=128 sits at the register cap: staging loads move to
        // the write point so their registers don't live across the compute
        constexpr bool EARLY = !(DO_DK && !DO_DV && D == 128);
        const int n_qt = (S - q_first) / QT;
        if (n_qt > 0) {
            stage_load(q_first);
            stage_write(0, q_first);
        }
        __syncthreads();

        for (int it = 0; it < n_qt; ++it) {
            const int q0 = q_first + it * QT;
            const int cur = it & 1;
            const bool last = (it + 1 == n_qt);
            if (EARLY && !last) stage_load(q0 + QT);

            // wave-skip: a q-tile entirely above this wave's diagonal
            const bool active = full_vis || (q0 + QT - 1 >= kv0w_u + kv_off);
            if (active) {
                // MASKED is a compile-time tag: sub-tiles wholly at or below
                // the wave's diagonal run the body without mask instructions
                auto qs_body = [&](int qs2c, auto masked_t) {
                    constexpr bool MASKED = decltype(masked_t)::value;
                    f32x16 st, dp;
#pragma unroll
                    for (int r = 0; r < 16; ++r) { st[r] = 0.f; dp[r] = 0.f; }
                    __builtin_amdgcn_s_setprio(1);
#pragma unroll
                    for (int c = 0; c < DCH; ++c) {
                        // St = Q·K^T: A = Q rows (row-major read), B = K regs
                        frag_ab aQ = *reinterpret_cast<const frag_ab*>(
                            &qs_lds[cur][sub_idx<D>(qs2c * 32 + l31,
                                                    c * 16 + 8 * hi)]);
                        st = MFMA_32x32x16(aQ, bK[c], st);
                        if (DO_DK) {
                            frag_ab aDO = *reinterpret_cast<const frag_ab*>(
                                &dos_lds[cur][sub_idx<D>(qs2c * 32 + l31,
                                                         c * 16 + 8 * hi)]);
                            dp = MFMA_32x32x16(aDO, bV[c], dp);  // dO·V^T
                        }
                    }
                    __builtin_amdgcn_s_setprio(0);
                    // softmax/dS phase. Register r is q row iq with
                    // jk - iq = dji - roff(r), roff(r) = 8*(r>>2) + (r&3).
                    // Every value is rounded exactly where it always was
                    // (st*scale2 and slope2*(jk-iq) each rounded, added, then
                    // -lse; dS scaled per element), so results are bitwise
                    // what the branchy form gave; only the work around them
                    // is gone. The position difference goes to float once
                    // per sub-tile: both are small integers, so fdji - roff
                    // is exact. The exponent is <= ~0 for live elements (lse
                    // is the row's log-sum), so the raw v_exp_f32 serves:
                    // results below 2^-126 flush to zero and vanish in P's
                    // bf16 rounding. Masked elements are selected away AFTER
                    // the exp (it may be +inf there), never multiplied.
                    const int dji = n_glob + kv_off - q0 - qs2c * 32 - 4 * hi;
                    const float fdji = (float)dji;
                    const bool all_live = !PEEL && full_vis;
                    // Row statistics: register r is q row 8*(r>>2) + (r&3)
                    // + 4*hi, so each group of four registers reads four
                    // consecutive floats with one ds_read_b128 (the scheduler
                    // moves the reads up as far as registers allow).
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const f32x4 l4 = *reinterpret_cast<const f32x4*>(
                            &lse_lds[cur][qs2c * 32 + 8 * g + 4 * hi]);
                        f32x4 d4 = {0.f, 0.f, 0.f, 0.f};
                        if (DO_DK)
                            d4 = *reinterpret_cast<const f32x4*>(
                                &dlt_lds[cur][qs2c * 32 + 8 * g + 4 * hi]);
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const int r = 4 * g + e;
                            const int roff = e + 8 * g;
                            const float z2 = mul2_add(
                                st[r], scale2, slope2, fdji - (float)roff);
                            float p = __builtin_amdgcn_exp2f(z2 - l4[e]);
                            if (MASKED)
                                p = (all_live || dji <= roff) ? p : 0.f;
                            st[r] = p;                               // P
                            if (DO_DK)
                                dp[r] = p * (dp[r] - d4[e]) * scale; // dS
                        }
                    }
                    // pack P and dS into B-fragments over the q axis
                    frag_ab pfrag[2], dsfrag[2];
#pragma unroll
                    for (int hf = 0; hf < 2; ++hf) {
                        if (DO_DV) pfrag[hf] = c_to_bfrag(st, hf);
                        if (DO_DK) dsfrag[hf] = c_to_bfrag(dp, hf);
                    }
                    // dV^T += dO^T·P  and  dK^T += Q^T·dS (transpose reads)
#pragma unroll
                    for (int dsb = 0; dsb < DSUB; ++dsb) {
                        __builtin_amdgcn_s_setprio(1);
#pragma unroll
                        for (int ksq = 0; ksq < 2; ++ksq) {
                            const int g0 = qs2c * 8 + 4 * ksq + 2 * hi;
                            const int dblk = 2 * dsb + (lq & 1);
                            if (DO_DV) {
                                union { frag_ab f; bf16x4 h[2]; } adot;
                                adot.h[0] = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
                                    (lds_bf16x4_p)&dos_lds[cur][
                                        sub_tile_base<D>(g0, dblk) + (lane & 15) * 4]);
                                adot.h[1] = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
                                    (lds_bf16x4_p)&dos_lds[cur][
                                        sub_tile_base<D>(g0 + 1, dblk) + (lane & 15) * 4]);
                                accDV[DO_DV ? dsb : 0] = MFMA_32x32x16(
                                    adot.f, pfrag[ksq], accDV[DO_DV ? dsb : 0]);
                            }
                            if (DO_DK && dsb >= DK0 && dsb < DK0 + NDSB) {
                                const int dblk_k = 2 * dsb + (lq & 1);
                                union { frag_ab f; bf16x4 h[2]; } aqt;
                                aqt.h[0] = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
                                    (lds_bf16x4_p)&qs_lds[cur][
                                        sub_tile_base<D>(g0, dblk_k) + (lane & 15) * 4]);
                                aqt.h[1] = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
                                    (lds_bf16x4_p)&qs_lds[cur][
                                        sub_tile_base<D>(g0 + 1, dblk_k) + (lane & 15) * 4]);
                                const int ai = DO_DK ? dsb - DK0 : 0;
                                accDK[ai] = MFMA_32x32x16(
                                    aqt.f, dsfrag[ksq], accDK[ai]);
                            }
                        }
                        __builtin_amdgcn_s_setprio(0);
                    }
                };
                // wave-uniform classification of one 32x32 sub-tile: none
                // of the wave's kv rows lies above the sub-tile's first q row
                auto qs_run = [&](int qs2c) {
                    if (PEEL &&
                        (full_vis || kv0w_u + 31 + kv_off <= q0 + qs2c * 32))
                        qs_body(qs2c, std::false_type{});
                    else
                        qs_body(qs2c, std::true_type{});
                };
                // rolled at D=128 (register cap) and in the 8-wave D=64 build,
                // where four unrolled bodies (2 sub-tiles x masked/mask-free)
                // spill 68 B
                if (D == 128 || WAVES == 8) {
#pragma unroll 1
                    for (int qs2c = 0; qs2c < 2; ++qs2c) qs_run(qs2c);
                } else {
                    qs_run(0);
                    qs_run(1);
                }
            }
            if (!last) {
                if (!EARLY) stage_load(q0 + QT);
                stage_write(cur ^ 1, q0 + QT);
            }
            __syncthreads();
        }
        __syncthreads();  // gq rotation reuses the LDS buffers
    }

    // epilogue: lane owns kv row n_glob; reg r is d = 8*(r>>2)+(r&3)+4*hi
    bf16* dkrow = dk + b * wb + h * wh + (int64_t)n_glob * ws;
    bf16* dvrow = dv + b * wb + h * wh + (int64_t)n_glob * ws;
#pragma unroll
    for (int dsb = 0; dsb < DSUB; ++dsb) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            union { __bf16 h4[4]; uint2 u; } wk2, wv2;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (DO_DK && dsb >= DK0 && dsb < DK0 + NDSB)
                    wk2.h4[r] = (__bf16)accDK[dsb - DK0][4 * g + r];
                if (DO_DV) wv2.h4[r] = (__bf16)accDV[dsb][4 * g + r];
            }
            if (DO_DK && dsb >= DK0 && dsb < DK0 + NDSB)
                *reinterpret_cast<uint2*>(dkrow + dsb * 32 + 8 * g + 4 * hi) = wk2.u;
            if (DO_DV)
                *reinterpret_cast<uint2*>(dvrow + dsb * 32 + 8 * g + 4 * hi) = wv2.u;
        }
    }
}

}  // namespace

// ======================================================================
// Host side: one selection table, one argument check, one launcher.
namespace {

struct AttnVariant {
    bool v2;     // the 32x32-MFMA kernels; false = the v1 fallback
    int waves;   // per workgroup
    int rows() const { return waves * (v2 ? 32 : 16); }  // per workgroup
};

// The selection table of the file header.  Forward and backward both launch
// what this returns, so they always tile a problem the same way.
AttnVariant select_variant(int64_t S, int64_t D) {
    TORCH_CHECK(D == 64 || D == 128,
                "attention: head dim must be 64 or 128, got ", D);
    TORCH_CHECK(S > 0 && S % 64 == 0,
                "attention: S must be a positive multiple of 64, got ", S);
    if (S % 128 != 0) return {false, 4};
    if (S % 256 != 0) return {true, 4};
    return {true, 8};
}

// a bf16 [.,.,.,D] device tensor of the given sizes, d contiguous
void check_operand(const char* who, const char* name, const torch::Tensor& t,
                   torch::IntArrayRef sizes) {
    TORCH_CHECK(t.is_cuda(), who, ": ", name, " must be on the GPU");
    TORCH_CHECK(t.scalar_type() == torch::kBFloat16, who, ": ", name,
                " must be bf16");
    TORCH_CHECK(t.sizes() == sizes, who, ": ", name, " has sizes ", t.sizes(),
                ", expected ", sizes);
    TORCH_CHECK(t.stride(3) == 1, who, ": last dim of ", name,
                " must be contiguous");
}

struct AttnDims {
    int B, H, Hkv, S, D;
    AttnVariant var;
};

// What every kernel assumes about q, k, v and slopes; shared by attn_fwd and
// attn_bwd_into, and done before anything is launched.
AttnDims check_qkv(const char* who, const torch::Tensor& q,
                   const torch::Tensor& k, const torch::Tensor& v,
                   const torch::Tensor& slopes, int64_t kv_off) {
    // a positive offset leaves the first rows without any visible key
    // (l = 0, o = 0 * inf) and no caller needs it; the lower bound keeps the
    // kernels' int position arithmetic far from overflow
    TORCH_CHECK(kv_off <= 0 && kv_off >= -(int64_t(1) << 30), who,
                ": kv_off must be in [-2^30, 0] (0 causal, (-S, 0) shifted "
                "causal, <= -S fully visible), got ", kv_off);
    TORCH_CHECK(q.dim() == 4 && k.dim() == 4, who,
                ": q and k must be [B, H, S, D]");
    const int64_t B = q.size(0), H = q.size(1), S = q.size(2), D = q.size(3);
    const int64_t Hkv = k.size(1);
    check_operand(who, "q", q, {B, H, S, D});
    check_operand(who, "k", k, {B, Hkv, S, D});
    check_operand(who, "v", v, {B, Hkv, S, D});
    TORCH_CHECK(Hkv > 0 && H % Hkv == 0, who,
                ": q heads must be a multiple of kv heads");
    TORCH_CHECK(slopes.is_cuda() && slopes.scalar_type() == torch::kFloat &&
                slopes.numel() == H && slopes.is_contiguous(), who,
                ": slopes must be ", H, " contiguous fp32 values on the GPU");
    return {(int)B, (int)H, (int)Hkv, (int)S, (int)D, select_variant(S, D)};
}

const bf16* bf16_in(const torch::Tensor& t) {
    return reinterpret_cast<const bf16*>(t.data_ptr());
}
bf16* bf16_out(const torch::Tensor& t) {
    return reinterpret_cast<bf16*>(t.data_ptr());
}
// batch, head and row strides, in the order every kernel takes them
std::tuple<int64_t, int64_t, int64_t> strides3(const torch::Tensor& t) {
    return {t.stride(0), t.stride(1), t.stride(2)};
}

// Launches `kernel` on `waves`-wave workgroups; `args` is a tuple in the
// kernel's parameter order.
template <typename... P, typename Args>
void launch(void (*kernel)(P...), dim3 grid, int waves, hipStream_t stream,
            const Args& args) {
    static_assert(sizeof...(P) == std::tuple_size<Args>::value,
                  "argument pack does not match the kernel's parameters");
    std::apply([&](auto... a) {
        hipLaunchKernelGGL(kernel, grid, dim3(waves * WAVE_SIZE), 0, stream,
                           static_cast<P>(a)...);
    }, args);
}

// Calls f(integral_constant<D>, integral_constant<waves>): the one place
// where the runtime head dim and wave count become template arguments.
template <typename F>
void with_d_waves(int D, int waves, F&& f) {
    auto with_waves = [&](auto d) {
        if (waves == 8) f(d, std::integral_constant<int, 8>{});
        else f(d, std::integral_constant<int, 4>{});
    };
    if (D == 64) with_waves(std::integral_constant<int, 64>{});
    else with_waves(std::integral_constant<int, 128>{});
}

}  // namespace

std::tuple<std::string, int64_t> attn_variant(int64_t S, int64_t D) {
    const AttnVariant var = select_variant(S, D);
    return {var.v2 ? "v2" : "v1", var.waves};
}

std::vector<torch::Tensor> attn_fwd(torch::Tensor q, torch::Tensor k,
                                    torch::Tensor v, torch::Tensor slopes,
                                    double scale, int64_t kv_off) {
    const AttnDims d = check_qkv("attn_fwd", q, k, v, slopes, kv_off);

    // O physically [B, S, H, D]: the model reshapes attention output back to
    // [B, S, H*D] for the dense projection — this layout makes that free.
    auto o_phys = torch::empty({d.B, d.S, d.H, d.D}, q.options());
    auto o = o_phys.permute({0, 2, 1, 3});
    auto lse = torch::empty({d.B, d.H, d.S}, q.options().dtype(torch::kFloat));

    const auto args = std::tuple_cat(
        std::make_tuple(bf16_in(q), bf16_in(k), bf16_in(v),
                        slopes.data_ptr<float>(), (float)scale,
                        bf16_out(o_phys), lse.data_ptr<float>(),
                        d.B, d.H, d.S, (int)kv_off, d.H / d.Hkv),
        strides3(q), strides3(k), strides3(v), strides3(o));
    const dim3 grid(d.S / d.var.rows(), d.H, d.B);
    auto stream = at::cuda::getCurrentCUDAStream();
    with_d_waves(d.D, d.var.waves, [&](auto dv_, auto wv_) {
        constexpr int DV = decltype(dv_)::value, WV = decltype(wv_)::value;
        if (d.var.v2) launch(attn_fwd_v2_kernel<DV, WV>, grid, WV, stream, args);
        else launch(attn_fwd_kernel<DV>, grid, WV, stream, args);
    });
    HIP_CHECK_LAUNCH();
    return {o, lse};
}

void attn_bwd_into(torch::Tensor dout, torch::Tensor q,
                   torch::Tensor k, torch::Tensor v,
                   torch::Tensor o, torch::Tensor lse,
                   torch::Tensor slopes, double scale,
                   torch::Tensor dq, torch::Tensor dk, torch::Tensor dv,
                   int64_t kv_off) {
    const AttnDims d = check_qkv("attn_bwd", q, k, v, slopes, kv_off);
    check_operand("attn_bwd", "dout", dout, q.sizes());
    check_operand("attn_bwd", "o", o, q.sizes());
    check_operand("attn_bwd", "dq", dq, q.sizes());
    check_operand("attn_bwd", "dk", dk, k.sizes());
    check_operand("attn_bwd", "dv", dv, k.sizes());
    // dk and dv must share a stride layout (one stride set feeds both writes)
    TORCH_CHECK(dk.strides() == dv.strides(),
                "attn_bwd: dk and dv must have the same strides");
    TORCH_CHECK(lse.is_cuda() && lse.scalar_type() == torch::kFloat &&
                lse.sizes() == torch::IntArrayRef({d.B, d.H, d.S}) &&
                lse.is_contiguous(),
                "attn_bwd: lse must be contiguous fp32 [B, H, S] on the GPU");
    auto delta = torch::empty({d.B, d.H, d.S},
                              q.options().dtype(torch::kFloat));

    const int64_t rows = (int64_t)d.B * d.H * d.S;
    const auto delta_args = std::tuple_cat(
        std::make_tuple(bf16_in(dout), bf16_in(o), delta.data_ptr<float>(),
                        rows, d.H, d.S),
        strides3(dout), strides3(o));
    // dq and dkdv kernels differ only in their outputs and output strides
    const auto inputs = std::make_tuple(
        bf16_in(dout), bf16_in(q), bf16_in(k), bf16_in(v),
        lse.data_ptr<float>(), delta.data_ptr<float>(),
        slopes.data_ptr<float>(), (float)scale);
    const auto dims_strides = std::tuple_cat(
        std::make_tuple(d.B, d.H, d.S, (int)kv_off, d.H / d.Hkv),
        strides3(dout), strides3(q), strides3(k), strides3(v));
    const auto dq_args = std::tuple_cat(
        inputs, std::make_tuple(bf16_out(dq)), dims_strides, strides3(dq));
    const auto dkdv_args = std::tuple_cat(
        inputs, std::make_tuple(bf16_out(dk), bf16_out(dv)), dims_strides,
        strides3(dk));

    const dim3 grid_delta((rows + 3) / 4);
    const dim3 grid_q(d.S / d.var.rows(), d.H, d.B);
    const dim3 grid_kv(d.S / d.var.rows(), d.Hkv, d.B);
    auto stream = at::cuda::getCurrentCUDAStream();
    with_d_waves(d.D, d.var.waves, [&](auto dv_, auto wv_) {
        constexpr int DV = decltype(dv_)::value, WV = decltype(wv_)::value;
        launch(attn_bwd_delta_kernel<DV>, grid_delta, 4, stream, delta_args);
        if (!d.var.v2) {
            launch(attn_bwd_dkdv_kernel<DV>, grid_kv, WV, stream, dkdv_args);
            launch(attn_bwd_dq_kernel<DV>, grid_q, WV, stream, dq_args);
            return;
        }
        launch(attn_bwd_dq_v2_kernel<DV, WV>, grid_q, WV, stream, dq_args);
        if constexpr (DV == 64) {
            launch(attn_bwd_dkdv_v2_kernel<64, WV, true, true, -1>,
                   grid_kv, WV, stream, dkdv_args);
        } else {
            // the fused kernel would spill at D=128 (256+144 registers
            // wanted): a dv-only pass plus two half-width dk passes (St
            // recomputed, +25% MFMA but no scratch traffic)
            launch(attn_bwd_dkdv_v2_kernel<128, WV, false, true, -1>,
                   grid_kv, WV, stream, dkdv_args);
            launch(attn_bwd_dkdv_v2_kernel<128, WV, true, false, 0>,
                   grid_kv, WV, stream, dkdv_args);
            launch(attn_bwd_dkdv_v2_kernel<128, WV, true, false, 1>,
                   grid_kv, WV, stream, dkdv_args);
        }
    });
    HIP_CHECK_LAUNCH();
}

std::vector<torch::Tensor> attn_bwd(torch::Tensor dout, torch::Tensor q,
                                    torch::Tensor k, torch::Tensor v,
                                    torch::Tensor o, torch::Tensor lse,
                                    torch::Tensor slopes, double scale,
                                    int64_t kv_off) {
    const int B = q.size(0), H = q.size(1), S = q.size(2), D = q.size(3);
    const int Hkv = k.size(1);
    // grads physically [B, S, H, D] (the layout the fused-qkv backward wants)
    auto dq_phys = torch::empty({B, S, H, D}, q.options());
    auto dk_phys = torch::empty({B, S, Hkv, D}, q.options());
    auto dv_phys = torch::empty({B, S, Hkv, D}, q.options());
    auto dq = dq_phys.permute({0, 2, 1, 3});
    auto dk = dk_phys.permute({0, 2, 1, 3});
    auto dv = dv_phys.permute({0, 2, 1, 3});
    attn_bwd_into(dout, q, k, v, o, lse, slopes, scale, dq, dk, dv, kv_off);
    return {dq, dk, dv};
}
