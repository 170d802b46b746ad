// Grouped expert GEMM for the MoE expert bank (gfx950, bf16 -> fp32 acc).
//
// One launch per pass walks the expert-sorted token buffer directly:
// expert e owns rows offsets[e] .. offsets[e+1]-1 of X / dY, ragged and
// unpadded, and every expert's [N,K] weight is read in place through a
// pointer table passed BY VALUE in the kernarg (E <= 64) -- no stacked
// weight bank, no transposed copies, no device-side table to go stale.
//
//   fwd    Y[r]  = X[r]  . W[e]^T (+ b[e])     contraction over K
//   dgrad  dX[r] = dY[r] . W[e]                contraction over N
//   wgrad  dW[e] = dY_e^T . X_e, db[e] = colsum(dY_e)   contraction over rows
//
// All three use the gemm.hip tile: 128 x BN output tile, 64-deep steps,
// 4 waves (2x2), mfma_f32_16x16x32_bf16, double-buffered LDS staged by
// global_load_lds.  Operands whose contraction index is NOT the contiguous
// one (W in dgrad, dY and X in wgrad) stay row-major in LDS and their MFMA
// fragments come out of ds_read_b64_tr_b16 (layout pinned by tr16_probe):
// lane 4q+p of a 16-lane group addresses row q, columns 4p..4p+3 of a
// [4][16] block and lane i receives column i, row q in element q.  Those
// reads sit in block-uniform control flow only (EXEC all ones).  The LDS
// images are bank-swizzled on the source address of the staging loads.
//
// Ragged edges:
//  * fwd/dgrad M-tiles start at the segment start, so the last tile of a
//    segment is partial: source rows are clamped to the segment's last row
//    (every global_load_lds lane has a valid address) and stores are
//    masked -- rows past the end belong to the next expert.
//  * wgrad contracts over the rows, so the tail of the last 64-row step
//    must contribute ZERO: loads are clamped for address validity, then the
//    tail rows of both LDS tiles are overwritten with zeros before use.
//  * offsets are clamped to [0,T] and made monotone in-kernel.
//  * the grid is an upper bound computed on the host from T and E (no
//    sync); surplus blocks leave before their first barrier.
//  * wgrad is one block per output tile looping over the whole segment in
//    order: no atomics, no split-K, bitwise repeatable.  Empty experts get
//    zeros for dW[e] and db[e].
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

#include "common.h"

namespace {

using bf16 = __hip_bfloat16;
using frag_ab = __attribute__((ext_vector_type(8))) __bf16;
using frag_cd = __attribute__((ext_vector_type(4))) float;
using bf16x4 = __attribute__((ext_vector_type(4))) __bf16;
using lds_bf16x4_p = __attribute__((address_space(3))) bf16x4*;

__device__ __forceinline__ frag_cd MFMA16(frag_ab a, frag_ab b, frag_cd c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

constexpr int MAX_EXPERTS = 64;
constexpr int BM = 128, BK = 64;
constexpr int NTHREADS = 256;  // 4 waves

struct WeightPtrs {
    const bf16* w[MAX_EXPERTS];
};

// XCD-aware bijective remap (see gemm.hip); identity on grids under 8.
__device__ __forceinline__ int xcd_remap(int wgid, int nwg) {
    const int q = nwg >> 3, r = nwg & 7;
    const int xcd = wgid & 7, idx = wgid >> 3;
    if (q > 0) {
        wgid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
    }
    return wgid;
}

__device__ __forceinline__ int clamp_off(int v, int T) {
    return v < 0 ? 0 : (v > T ? T : v);
}

// (expert, first row, live rows) of 128-row M-tile `mt`: tiles lie only
// inside the clamped, monotone segments.  e < 0 marks a surplus block of
// the host's grid bound.  Block-uniform.
struct MTile {
    int e, row0, rows_valid;
};

__device__ __forceinline__ MTile locate_m_tile(const int* __restrict__ offsets,
                                               int mt, int T, int E) {
    MTile t{-1, 0, 0};
    int acc = 0;
    int lo = clamp_off(offsets[0], T);
    for (int i = 0; i < E; ++i) {
        int hi = clamp_off(offsets[i + 1], T);
        hi = hi > lo ? hi : lo;
        const int tiles = (hi - lo + BM - 1) / BM;
        if (mt < acc + tiles) {
            t.e = i;
            t.row0 = lo + (mt - acc) * BM;
            t.rows_valid = hi - t.row0 < BM ? hi - t.row0 : BM;
            break;
        }
        acc += tiles;
        lo = hi;
    }
    return t;
}

// LDS bank swizzles.  global_load_lds writes lane-linear, so the images
// are swizzled on the SOURCE side: LDS position (row, physical block p)
// holds the tile's logical block p ^ f(row) of that row.
//
// Row-read images ([.][64], fragments read with ds_read_b128): rows are
// 128 B, so rows r and r+2 share banks; XOR the 16-B slot with (row>>1)&7.
__device__ __forceinline__ int row_swz(int row) { return (row >> 1) & 7; }
// Transposed-read images ([.][COLS], ds_read_b64_tr_b16): one half-wave
// reads 32-B blocks of rows {0..3, 8..11} (+4, +16) of one 16-column block;
// unswizzled they all land on the same 8 banks.  XOR the 32-B block index
// so the 8 rows take 8 different blocks.  f(row) == f(row + 4) for rows
// with bit 2 clear, which lets a fragment's two reads share one address.
template <int COLS>
__device__ __forceinline__ int tr_swz(int row) {
    static_assert(COLS == 128 || COLS == 64, "tile width");
    return COLS == 128 ? ((row & 3) | ((row >> 1) & 4))
                       : (((row >> 1) & 1) | ((row >> 2) & 2));
}

// Stage a [ROWS][COLS] bf16 tile into a lane-linear LDS image with
// global_load_lds: chunk c is 1 KiB (512 elements), lane l supplies the
// source of elements [512c + 8l, 512c + 8l + 8).  Source rows are clamped
// to `row_clamp` so every lane reads inside the caller's segment.  TR picks
// the swizzle of the image's reader (the column permutation stays inside
// the row, so it never changes which rows or columns are touched).
template <int ROWS, int COLS, bool TR>
__device__ __forceinline__ void stage_tile(bf16* lds, const bf16* src,
                                           int64_t ld, int row_clamp,
                                           int wave, int lane) {
    static_assert(TR || COLS == 64, "row-read images are 64 wide");
    constexpr int CHUNKS = ROWS * COLS / 512;
    static_assert(CHUNKS % 4 == 0, "tile must split over 4 waves");
#pragma unroll
    for (int i = 0; i < CHUNKS / 4; ++i) {
        const int c = wave * (CHUNKS / 4) + i;
        const int el = c * 512 + lane * 8;
        int row = el / COLS;
        const int pc = el % COLS;
        const int col = TR
            ? ((((pc >> 4) ^ tr_swz<COLS>(row)) << 4) | (pc & 15))
            : (((pc >> 3) ^ row_swz(row)) << 3);
        row = row < row_clamp ? row : row_clamp;
        __builtin_amdgcn_global_load_lds(
            (const __attribute__((address_space(1))) unsigned int*)(
                (const void*)(src + (int64_t)row * ld + col)),
            (__attribute__((address_space(3))) unsigned int*)(
                (void*)&lds[c * 512]),
            16, 0, 0);
    }
}

// MFMA fragment whose 8 contraction elements are 8 consecutive ROWS of a
// row-major [.][LD] LDS image (hardware transpose read): rows
// row0 + 8*lgrp + 0..7 (row0 % 32 == 0), columns c .. c+15 (c % 16 == 0).
template <int LD>
__device__ __forceinline__ frag_ab read_frag_tr(const bf16* img, int row0,
                                                int c, int lgrp, int lcol) {
    union { frag_ab f; bf16x4 h[2]; } v;
    const int row = row0 + 8 * lgrp + (lcol >> 2);
    const bf16* p = img + row * LD + (((c >> 4) ^ tr_swz<LD>(row)) << 4) +
                    4 * (lcol & 3);
    v.h[0] = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4_p)p);
    v.h[1] = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
        (lds_bf16x4_p)(p + 4 * LD));
    return v.f;
}

// Fragment of a row-read [.][64] image: row `row`, elements 8*slot .. +7.
__device__ __forceinline__ frag_ab read_frag_row(const bf16* img, int row,
                                                 int slot) {
    return *reinterpret_cast<const frag_ab*>(
        img + row * BK + ((slot ^ row_swz(row)) << 3));
}

// ------------------------------------------------------------ fwd / dgrad
// C[r, :] = A[r, :] . op(W[e]) for the rows r of expert e.
//   TRANS_B = false: W[e] is [NOUT, KC], contraction-contiguous (forward)
//   TRANS_B = true : W[e] is [KC, NOUT], output-contiguous       (dgrad)
template <bool TRANS_B, int BN, bool BIAS>
__global__ __launch_bounds__(NTHREADS)
void grouped_gemm_kernel(const bf16* __restrict__ A, const WeightPtrs wp,
                         const int* __restrict__ offsets,
                         const float* __restrict__ bias,
                         bf16* __restrict__ C, int T, int E, int KC, int NOUT,
                         int n_tiles_n) {
    constexpr int NF = BN / 32;  // 16-col fragments per wave
    const int wgid = xcd_remap(blockIdx.x, gridDim.x);
    const int mt = wgid / n_tiles_n;
    const int tn = wgid % n_tiles_n;

    const MTile t = locate_m_tile(offsets, mt, T, E);
    const int e = t.e, row0 = t.row0, rows_valid = t.rows_valid;
    if (e < 0) return;  // surplus block of the host's upper bound

    __shared__ __attribute__((aligned(16))) bf16 a_t[2][BM * BK];
    __shared__ __attribute__((aligned(16))) bf16 b_t[2][BN * BK];

    const int tid = threadIdx.x;
    const int wave = tid / WAVE_SIZE;
    const int lane = tid % WAVE_SIZE;
    const int lgrp = lane >> 4, lcol = lane & 15;
    const int wr = wave >> 1, wn = wave & 1;  // 2x2 waves of 64 x BN/2

    frag_cd acc[4][NF];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < NF; ++j) acc[i][j] = frag_cd{0.f, 0.f, 0.f, 0.f};

    const bf16* __restrict__ W = wp.w[e];
    const bf16* a_base = A + (int64_t)row0 * KC;
    const int64_t col0 = (int64_t)tn * BN;
    auto stage = [&](int buf, int kt) {
        const int64_t k0 = (int64_t)kt * BK;
        stage_tile<BM, BK, false>(a_t[buf], a_base + k0, KC, rows_valid - 1, wave,
                           lane);
        if (TRANS_B) {
            stage_tile<BK, BN, true>(b_t[buf], W + k0 * NOUT + col0, NOUT,
                                     BK - 1, wave, lane);
        } else {
            stage_tile<BN, BK, false>(b_t[buf], W + col0 * KC + k0, KC,
                                      BN - 1, wave, lane);
        }
    };

    const int n_kt = KC / BK;
    stage(0, 0);
    __syncthreads();  // drains the glds (vmcnt(0))

    int buf = 0;
    for (int kt = 0; kt < n_kt; ++kt) {
        if (kt + 1 < n_kt) stage(buf ^ 1, kt + 1);
#pragma unroll
        for (int kk = 0; kk < BK / 32; ++kk) {
            frag_ab av[4];
#pragma unroll
            for (int mf = 0; mf < 4; ++mf) {
                av[mf] = read_frag_row(a_t[buf], wr * 64 + mf * 16 + lcol,
                                       kk * 4 + lgrp);
            }
            __builtin_amdgcn_s_setprio(1);
#pragma unroll
            for (int nf = 0; nf < NF; ++nf) {
                const int c = wn * (BN / 2) + nf * 16;
                frag_ab bv;
                if (TRANS_B) {
                    bv = read_frag_tr<BN>(b_t[buf], kk * 32, c, lgrp, lcol);
                } else {
                    bv = read_frag_row(b_t[buf], c + lcol, kk * 4 + lgrp);
                }
#pragma unroll
                for (int mf = 0; mf < 4; ++mf) {
                    acc[mf][nf] = MFMA16(av[mf], bv, acc[mf][nf]);
                }
            }
            __builtin_amdgcn_s_setprio(0);
        }
        __syncthreads();
        buf ^= 1;
    }

    // epilogue: row = 4*lgrp + r within each 16x16 fragment; rows past the
    // segment end are the next expert's and are never written
    bf16* c_base = C + (int64_t)row0 * NOUT;
#pragma unroll
    for (int nf = 0; nf < NF; ++nf) {
        const int64_t col = col0 + wn * (BN / 2) + nf * 16 + lcol;
        float bv = 0.f;
        if (BIAS) bv = bias[(int64_t)e * NOUT + col];
#pragma unroll
        for (int mf = 0; mf < 4; ++mf) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = wr * 64 + mf * 16 + 4 * lgrp + r;
                if (row < rows_valid) {
                    c_base[(int64_t)row * NOUT + col] =
                        (bf16)(acc[mf][nf][r] + bv);
                }
            }
        }
    }
}

// ------------------------------------------------------- gated (GLU) bank
// Gated experts: h = silu(x . Wg[e]^T) * (x . Wu[e]^T).
//
// Forward: a block owns 128 rows x 64 output columns and computes BOTH
// products for them from one staged X tile.  Its 128-row B image holds the
// 64 gate rows and the 64 up rows of the weights interleaved in groups of
// 32 -- [g 0-31 | u 0-31 | g 32-63 | u 32-63] -- so wave column wn has gate
// in fragments nf = 0,1 and up in nf = 2,3 for the same 32 output columns:
// acc[mf][nf][r] and acc[mf][nf + 2][r] are the gate and the up value of
// one output element, in the same lane.  The epilogue needs no LDS and no
// cross-lane traffic.  Every element is accumulated by the MFMA sequence
// grouped_gemm_kernel<false, 128, false> runs for it, so g and u are
// bitwise the two plain forwards; h is formed from the ROUNDED g and u
// with silu_mul.hip's formula, so the saved g, u define the forward exactly.
__device__ __forceinline__ float glu_silu(float x) {
    return x / (1.0f + __expf(-x));
}

template <bool SAVE_GU>
__global__ __launch_bounds__(NTHREADS)
void grouped_glu_fwd_kernel(const bf16* __restrict__ X, const WeightPtrs wg,
                            const WeightPtrs wu,
                            const int* __restrict__ offsets,
                            bf16* __restrict__ H, bf16* __restrict__ G,
                            bf16* __restrict__ U, int T, int E, int K, int I,
                            int n_tiles_n) {
    constexpr int BNO = 64;  // output columns per block
    constexpr int SUB = 32;  // rows per gate / up sub-image
    const int wgid = xcd_remap(blockIdx.x, gridDim.x);
    const int mt = wgid / n_tiles_n;
    const int tn = wgid % n_tiles_n;

    const MTile t = locate_m_tile(offsets, mt, T, E);
    const int e = t.e, row0 = t.row0, rows_valid = t.rows_valid;
    if (e < 0) return;  // surplus block of the host's upper bound

    __shared__ __attribute__((aligned(16))) bf16 a_t[2][BM * BK];
    __shared__ __attribute__((aligned(16))) bf16 b_t[2][2 * BNO * BK];

    const int tid = threadIdx.x;
    const int wave = tid / WAVE_SIZE;
    const int lane = tid % WAVE_SIZE;
    const int lgrp = lane >> 4, lcol = lane & 15;
    const int wr = wave >> 1, wn = wave & 1;  // 2x2 waves of 64 x (32g + 32u)

    frag_cd acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = frag_cd{0.f, 0.f, 0.f, 0.f};

    const int64_t col0 = (int64_t)tn * BNO;
    const bf16* a_base = X + (int64_t)row0 * K;
    const bf16* __restrict__ Wg = wg.w[e] + col0 * K;
    const bf16* __restrict__ Wu = wu.w[e] + col0 * K;
    auto stage = [&](int buf, int kt) {
        const int64_t k0 = (int64_t)kt * BK;
        stage_tile<BM, BK, false>(a_t[buf], a_base + k0, K, rows_valid - 1,
                                  wave, lane);
        // sub-images start at multiples of 32 rows: row_swz is unchanged
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            stage_tile<SUB, BK, false>(b_t[buf] + (2 * s) * SUB * BK,
                                       Wg + (int64_t)s * SUB * K + k0, K,
                                       SUB - 1, wave, lane);
            stage_tile<SUB, BK, false>(b_t[buf] + (2 * s + 1) * SUB * BK,
                                       Wu + (int64_t)s * SUB * K + k0, K,
                                       SUB - 1, wave, lane);
        }
    };

    const int n_kt = K / BK;
    stage(0, 0);
    __syncthreads();  // drains the glds (vmcnt(0))

    int buf = 0;
    for (int kt = 0; kt < n_kt; ++kt) {
        if (kt + 1 < n_kt) stage(buf ^ 1, kt + 1);
#pragma unroll
        for (int kk = 0; kk < BK / 32; ++kk) {
            frag_ab av[4];
#pragma unroll
            for (int mf = 0; mf < 4; ++mf) {
                av[mf] = read_frag_row(a_t[buf], wr * 64 + mf * 16 + lcol,
                                       kk * 4 + lgrp);
            }
            __builtin_amdgcn_s_setprio(1);
#pragma unroll
            for (int nf = 0; nf < 4; ++nf) {
                const frag_ab bv = read_frag_row(
                    b_t[buf], wn * 64 + nf * 16 + lcol, kk * 4 + lgrp);
#pragma unroll
                for (int mf = 0; mf < 4; ++mf) {
                    acc[mf][nf] = MFMA16(av[mf], bv, acc[mf][nf]);
                }
            }
            __builtin_amdgcn_s_setprio(0);
        }
        __syncthreads();
        buf ^= 1;
    }

    // epilogue: gate in nf, up in nf + 2; rows past the segment end are the
    // next expert's and are never written
    const int64_t out0 = (int64_t)row0 * I;
#pragma unroll
    for (int nf = 0; nf < 2; ++nf) {
        const int64_t col = col0 + wn * SUB + nf * 16 + lcol;
#pragma unroll
        for (int mf = 0; mf < 4; ++mf) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = wr * 64 + mf * 16 + 4 * lgrp + r;
                if (row < rows_valid) {
                    // "+ 0.f" is the bias-free forward's rounding input
                    const bf16 g = (bf16)(acc[mf][nf][r] + 0.f);
                    const bf16 u = (bf16)(acc[mf][nf + 2][r] + 0.f);
                    const int64_t o = out0 + (int64_t)row * I + col;
                    if (SAVE_GU) {
                        G[o] = g;
                        U[o] = u;
                    }
                    H[o] = __float2bfloat16(glu_silu(__bfloat162float(g)) *
                                            __bfloat162float(u));
                }
            }
        }
    }
}

// dX[r] = dg[r] . Wg[e] + du[r] . Wu[e]: the dgrad K loop run twice, over
// (dg, Wg) then (du, Wu), into ONE fp32 accumulator -- one launch and one
// rounding instead of two dgrads and a bf16 add.
template <int BN>
__global__ __launch_bounds__(NTHREADS)
void grouped_glu_dgrad_kernel(const bf16* __restrict__ dG,
                              const bf16* __restrict__ dU,
                              const WeightPtrs wg, const WeightPtrs wu,
                              const int* __restrict__ offsets,
                              bf16* __restrict__ dX, int T, int E, int I,
                              int K, int n_tiles_n) {
    constexpr int NF = BN / 32;  // 16-col fragments per wave
    const int wgid = xcd_remap(blockIdx.x, gridDim.x);
    const int mt = wgid / n_tiles_n;
    const int tn = wgid % n_tiles_n;

    const MTile t = locate_m_tile(offsets, mt, T, E);
    const int e = t.e, row0 = t.row0, rows_valid = t.rows_valid;
    if (e < 0) return;  // surplus block of the host's upper bound

    __shared__ __attribute__((aligned(16))) bf16 a_t[2][BM * BK];
    __shared__ __attribute__((aligned(16))) bf16 b_t[2][BK * BN];

    const int tid = threadIdx.x;
    const int wave = tid / WAVE_SIZE;
    const int lane = tid % WAVE_SIZE;
    const int lgrp = lane >> 4, lcol = lane & 15;
    const int wr = wave >> 1, wn = wave & 1;  // 2x2 waves of 64 x BN/2

    frag_cd acc[4][NF];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < NF; ++j) acc[i][j] = frag_cd{0.f, 0.f, 0.f, 0.f};

    const int64_t col0 = (int64_t)tn * BN;
    const int n_kt = I / BK;  // steps per product
    const bf16* ag = dG + (int64_t)row0 * I;
    const bf16* au = dU + (int64_t)row0 * I;
    const bf16* __restrict__ Wg = wg.w[e] + col0;
    const bf16* __restrict__ Wu = wu.w[e] + col0;
    auto stage = [&](int buf, int st) {  // step st of 2 * n_kt; uniform
        const bool up = st >= n_kt;
        const int64_t k0 = (int64_t)(up ? st - n_kt : st) * BK;
        stage_tile<BM, BK, false>(a_t[buf], (up ? au : ag) + k0, I,
                                  rows_valid - 1, wave, lane);
        stage_tile<BK, BN, true>(b_t[buf], (up ? Wu : Wg) + k0 * K, K, BK - 1,
                                 wave, lane);
    };

    stage(0, 0);
    __syncthreads();  // drains the glds (vmcnt(0))

    int buf = 0;
    for (int st = 0; st < 2 * n_kt; ++st) {
        if (st + 1 < 2 * n_kt) stage(buf ^ 1, st + 1);
#pragma unroll
        for (int kk = 0; kk < BK / 32; ++kk) {
            frag_ab av[4];
#pragma unroll
            for (int mf = 0; mf < 4; ++mf) {
                av[mf] = read_frag_row(a_t[buf], wr * 64 + mf * 16 + lcol,
                                       kk * 4 + lgrp);
            }
            __builtin_amdgcn_s_setprio(1);
#pragma unroll
            for (int nf = 0; nf < NF; ++nf) {
                const frag_ab bv = read_frag_tr<BN>(
                    b_t[buf], kk * 32, wn * (BN / 2) + nf * 16, lgrp, lcol);
#pragma unroll
                for (int mf = 0; mf < 4; ++mf) {
                    acc[mf][nf] = MFMA16(av[mf], bv, acc[mf][nf]);
                }
            }
            __builtin_amdgcn_s_setprio(0);
        }
        __syncthreads();
        buf ^= 1;
    }

    bf16* c_base = dX + (int64_t)row0 * K;
#pragma unroll
    for (int nf = 0; nf < NF; ++nf) {
        const int64_t col = col0 + wn * (BN / 2) + nf * 16 + lcol;
#pragma unroll
        for (int mf = 0; mf < 4; ++mf) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = wr * 64 + mf * 16 + 4 * lgrp + r;
                if (row < rows_valid) {
                    c_base[(int64_t)row * K + col] = (bf16)acc[mf][nf][r];
                }
            }
        }
    }
}

// ------------------------------------------------------------------ wgrad
// dW[e][n, k] = sum_r dY[r, n] X[r, k] over the rows of expert e; one block
// per (e, 128-row n tile, BKO-col k tile), looping over the segment in
// 64-row steps.  Blocks of k-tile 0 also reduce db[e][n] = sum_r dY[r, n]
// from the dY tile they already hold.
template <int BKO>
__global__ __launch_bounds__(NTHREADS)
void grouped_wgrad_kernel(const bf16* __restrict__ dY,
                          const bf16* __restrict__ X,
                          const int* __restrict__ offsets,
                          bf16* __restrict__ dW, float* __restrict__ db,
                          int T, int E, int N, int K) {
    constexpr int BR = 64;        // contraction rows per step
    constexpr int NF = BKO / 32;  // 16-col fragments per wave
    const int nn = N / BM, nk = K / BKO;
    // The XCD remap is applied WITHIN each expert's tiles: a block's cost is
    // its expert's row count, so handing one XCD a contiguous chunk of the
    // whole grid would give it whole experts and serialise a skewed routing
    // on one eighth of the chip.
    const int per_e = nn * nk;
    const int e = blockIdx.x / per_e;
    const int wgid = xcd_remap(blockIdx.x % per_e, per_e);
    const int tk = wgid % nk;
    const int tn = wgid / nk;

    int lo = clamp_off(offsets[0], T), hi = lo;
    for (int i = 0; i <= e; ++i) {
        lo = hi;
        hi = clamp_off(offsets[i + 1], T);
        hi = hi > lo ? hi : lo;
    }
    const int cnt = hi - lo;

    __shared__ __attribute__((aligned(16))) bf16 a_t[2][BR * BM];   // dY
    __shared__ __attribute__((aligned(16))) bf16 b_t[2][BR * BKO];  // X

    const int tid = threadIdx.x;
    const int wave = tid / WAVE_SIZE;
    const int lane = tid % WAVE_SIZE;
    const int lgrp = lane >> 4, lcol = lane & 15;
    const int wr = wave >> 1, wn = wave & 1;  // 2x2 waves of 64 x BKO/2

    frag_cd acc[4][NF];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < NF; ++j) acc[i][j] = frag_cd{0.f, 0.f, 0.f, 0.f};

    const int64_t n0 = (int64_t)tn * BM, k0 = (int64_t)tk * BKO;
    const bool do_db = (db != nullptr) && tk == 0;
    float db_acc = 0.f;

    const int n_rt = (cnt + BR - 1) / BR;
    auto stage = [&](int buf, int rt) {
        const int64_t r0 = (int64_t)lo + (int64_t)rt * BR;
        const int left = cnt - rt * BR;  // >= 1
        const int clampr = (left < BR ? left : BR) - 1;
        stage_tile<BR, BM, true>(a_t[buf], dY + r0 * N + n0, N, clampr, wave,
                                lane);
        stage_tile<BR, BKO, true>(b_t[buf], X + r0 * K + k0, K, clampr, wave,
                                 lane);
    };

    if (n_rt > 0) {  // block-uniform
        stage(0, 0);
        __syncthreads();
    }
    int buf = 0;
    for (int rt = 0; rt < n_rt; ++rt) {
        if (rt + 1 < n_rt) stage(buf ^ 1, rt + 1);
        const int left = cnt - rt * BR;
        if (left < BR) {
            // contraction tail: the clamped rows hold real data of this
            // segment's last row; they must contribute zero
            const frag_ab z = {0, 0, 0, 0, 0, 0, 0, 0};
            for (int i = left * (BM / 8) + tid; i < BR * (BM / 8);
                 i += NTHREADS)
                *reinterpret_cast<frag_ab*>(&a_t[buf][i * 8]) = z;
            for (int i = left * (BKO / 8) + tid; i < BR * (BKO / 8);
                 i += NTHREADS)
                *reinterpret_cast<frag_ab*>(&b_t[buf][i * 8]) = z;
            __syncthreads();
        }
        if (do_db) {
            // thread t: column t%128, rows [32*(t/128), +32) of the step
            const int c = tid & (BM - 1), rh = (tid >> 7) * (BR / 2);
#pragma unroll 8
            for (int r = 0; r < BR / 2; ++r) {
                const int row = rh + r;
                db_acc += __bfloat162float(a_t[buf][
                    row * BM + (((c >> 4) ^ tr_swz<BM>(row)) << 4) + (c & 15)]);
            }
        }
#pragma unroll
        for (int kk = 0; kk < BR / 32; ++kk) {
            frag_ab av[4];
#pragma unroll
            for (int mf = 0; mf < 4; ++mf) {
                av[mf] = read_frag_tr<BM>(a_t[buf], kk * 32,
                                          wr * 64 + mf * 16, lgrp, lcol);
            }
            __builtin_amdgcn_s_setprio(1);
#pragma unroll
            for (int nf = 0; nf < NF; ++nf) {
                frag_ab bv = read_frag_tr<BKO>(
                    b_t[buf], kk * 32, wn * (BKO / 2) + nf * 16, lgrp, lcol);
#pragma unroll
                for (int mf = 0; mf < 4; ++mf) {
                    acc[mf][nf] = MFMA16(av[mf], bv, acc[mf][nf]);
                }
            }
            __builtin_amdgcn_s_setprio(0);
        }
        __syncthreads();
        buf ^= 1;
    }

    if (do_db) {
        // fixed-order two-way combine through LDS (tiles are free now)
        float* red = reinterpret_cast<float*>(&a_t[0][0]);
        if (tid >= BM) red[tid - BM] = db_acc;
        __syncthreads();
        if (tid < BM) db[(int64_t)e * N + n0 + tid] = db_acc + red[tid];
    }

    bf16* c_base = dW + ((int64_t)e * N + n0) * K + k0;
#pragma unroll
    for (int nf = 0; nf < NF; ++nf) {
        const int col = wn * (BKO / 2) + nf * 16 + lcol;
#pragma unroll
        for (int mf = 0; mf < 4; ++mf) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = wr * 64 + mf * 16 + 4 * lgrp + r;
                c_base[(int64_t)row * K + col] = (bf16)acc[mf][nf][r];
            }
        }
    }
}

void check_offsets(const torch::Tensor& offsets, const torch::Tensor& like,
                   int64_t E) {
    TORCH_CHECK(offsets.is_cuda() && offsets.device() == like.device(),
                "grouped_gemm: offsets must live on the operands' device");
    TORCH_CHECK(offsets.scalar_type() == torch::kInt32 &&
                    offsets.dim() == 1 && offsets.is_contiguous(),
                "grouped_gemm: offsets must be a contiguous int32 vector");
    TORCH_CHECK(offsets.numel() == E + 1,
                "grouped_gemm: offsets must have E+1 entries");
}

void check_rows(const torch::Tensor& t, const char* name) {
    TORCH_CHECK(t.is_cuda() && t.dim() == 2, "grouped_gemm: ", name,
                " must be a 2-D device tensor");
    TORCH_CHECK(t.scalar_type() == torch::kBFloat16, "grouped_gemm: ", name,
                " must be bf16");
    TORCH_CHECK(t.is_contiguous(), "grouped_gemm: ", name,
                " must be contiguous");
    TORCH_CHECK(t.size(0) < (int64_t)1 << 31, "grouped_gemm: too many rows");
}

// Validates the bank and fills the by-value pointer table.
void collect_weights(const std::vector<torch::Tensor>& weights,
                     const torch::Tensor& like, WeightPtrs& wp, int64_t& N,
                     int64_t& K) {
    const int64_t E = (int64_t)weights.size();
    TORCH_CHECK(E >= 1 && E <= MAX_EXPERTS, "grouped_gemm: 1 <= E <= ",
                MAX_EXPERTS, " experts, got ", E);
    N = weights[0].size(0);
    K = weights[0].size(1);
    for (int64_t e = 0; e < E; ++e) {
        const auto& w = weights[e];
        TORCH_CHECK(w.is_cuda() && w.device() == like.device() &&
                        w.dim() == 2 && w.scalar_type() == torch::kBFloat16 &&
                        w.is_contiguous(),
                    "grouped_gemm: every weight must be a contiguous 2-D "
                    "bf16 tensor on the operands' device");
        TORCH_CHECK(w.size(0) == N && w.size(1) == K,
                    "grouped_gemm: all weights must share one [N,K] shape");
        wp.w[e] = reinterpret_cast<const bf16*>(w.data_ptr());
    }
    for (int64_t e = E; e < MAX_EXPERTS; ++e) wp.w[e] = nullptr;
    TORCH_CHECK(K % 64 == 0 && N % 128 == 0,
                "grouped_gemm: needs K % 64 == 0 and N % 128 == 0, got N=", N,
                " K=", K);
}

// upper bound on the number of 128-row M-tiles over all segments: every
// non-empty segment adds at most one partial tile, and no tile is empty
int64_t m_tiles_bound(int64_t T, int64_t E) {
    const int64_t ub = T / BM + E;
    return ub < T ? ub : T;
}

}  // namespace

torch::Tensor grouped_gemm_fwd(torch::Tensor X,
                               std::vector<torch::Tensor> weights,
                               torch::Tensor offsets,
                               c10::optional<torch::Tensor> bias) {
    check_rows(X, "X");
    WeightPtrs wp;
    int64_t N, K;
    collect_weights(weights, X, wp, N, K);
    const int64_t E = (int64_t)weights.size(), T = X.size(0);
    TORCH_CHECK(X.size(1) == K, "grouped_gemm_fwd: X is [T,", X.size(1),
                "] but weights are [", N, ",", K, "]");
    check_offsets(offsets, X, E);
    torch::Tensor bias_f;
    const bool has_bias = bias.has_value();
    if (has_bias) {
        TORCH_CHECK(bias->is_cuda() && bias->device() == X.device() &&
                        bias->dim() == 2 && bias->size(0) == E &&
                        bias->size(1) == N,
                    "grouped_gemm_fwd: bias must be [E,N] on X's device");
        bias_f = bias->to(torch::kFloat).contiguous();
    }
    auto Y = torch::empty({T, N}, X.options());
    if (T == 0) return Y;
    const int64_t n_tiles_n = N / 128;
    const int64_t grid = m_tiles_bound(T, E) * n_tiles_n;
    TORCH_CHECK(grid < (int64_t)1 << 31, "grouped_gemm_fwd: grid too large");
    auto stream = at::cuda::getCurrentCUDAStream();
#define LAUNCH(BIASV)                                                         \
    hipLaunchKernelGGL((grouped_gemm_kernel<false, 128, BIASV>),              \
        dim3((unsigned)grid), dim3(NTHREADS), 0, stream,                      \
        reinterpret_cast<const bf16*>(X.data_ptr()), wp,                      \
        offsets.data_ptr<int>(),                                              \
        has_bias ? bias_f.data_ptr<float>() : nullptr,                        \
        reinterpret_cast<bf16*>(Y.data_ptr()), (int)T, (int)E, (int)K,        \
        (int)N, (int)n_tiles_n)
    if (has_bias) LAUNCH(true);
    else LAUNCH(false);
#undef LAUNCH
    HIP_CHECK_LAUNCH();
    return Y;
}

torch::Tensor grouped_gemm_dgrad(torch::Tensor dY,
                                 std::vector<torch::Tensor> weights,
                                 torch::Tensor offsets) {
    check_rows(dY, "dY");
    WeightPtrs wp;
    int64_t N, K;
    collect_weights(weights, dY, wp, N, K);
    const int64_t E = (int64_t)weights.size(), T = dY.size(0);
    TORCH_CHECK(dY.size(1) == N, "grouped_gemm_dgrad: dY is [T,", dY.size(1),
                "] but weights are [", N, ",", K, "]");
    check_offsets(offsets, dY, E);
    auto dX = torch::empty({T, K}, dY.options());
    if (T == 0) return dX;
    // output columns run over K, which is only a multiple of 64
    const int bn = (K % 128 == 0) ? 128 : 64;
    const int64_t n_tiles_n = K / bn;
    const int64_t grid = m_tiles_bound(T, E) * n_tiles_n;
    TORCH_CHECK(grid < (int64_t)1 << 31, "grouped_gemm_dgrad: grid too large");
    auto stream = at::cuda::getCurrentCUDAStream();
#define LAUNCH(BNV)                                                           \
    hipLaunchKernelGGL((grouped_gemm_kernel<true, BNV, false>),               \
        dim3((unsigned)grid), dim3(NTHREADS), 0, stream,                      \
        reinterpret_cast<const bf16*>(dY.data_ptr()), wp,                     \
        offsets.data_ptr<int>(), nullptr,                                     \
        reinterpret_cast<bf16*>(dX.data_ptr()), (int)T, (int)E, (int)N,       \
        (int)K, (int)n_tiles_n)
    if (bn == 128) LAUNCH(128);
    else LAUNCH(64);
#undef LAUNCH
    HIP_CHECK_LAUNCH();
    return dX;
}

std::vector<torch::Tensor> grouped_gemm_wgrad(torch::Tensor dY,
                                              torch::Tensor X,
                                              torch::Tensor offsets,
                                              int64_t E,
                                              bool want_bias_grad) {
    check_rows(dY, "dY");
    check_rows(X, "X");
    TORCH_CHECK(X.device() == dY.device() && X.size(0) == dY.size(0),
                "grouped_gemm_wgrad: dY and X must share rows and device");
    TORCH_CHECK(E >= 1 && E <= MAX_EXPERTS, "grouped_gemm: 1 <= E <= ",
                MAX_EXPERTS, " experts, got ", E);
    const int64_t T = X.size(0), N = dY.size(1), K = X.size(1);
    TORCH_CHECK(K % 64 == 0 && N % 128 == 0,
                "grouped_gemm: needs K % 64 == 0 and N % 128 == 0, got N=", N,
                " K=", K);
    check_offsets(offsets, X, E);
    torch::Tensor dW, db;
    if (T == 0) {  // every expert is empty: zeros, no launch
        dW = torch::zeros({E, N, K}, X.options());
        if (want_bias_grad)
            db = torch::zeros({E, N}, X.options().dtype(torch::kFloat));
        else
            db = torch::empty({0}, X.options().dtype(torch::kFloat));
        return {dW, db};
    }
    dW = torch::empty({E, N, K}, X.options());
    db = want_bias_grad
             ? torch::empty({E, N}, X.options().dtype(torch::kFloat))
             : torch::empty({0}, X.options().dtype(torch::kFloat));
    const int bko = (K % 128 == 0) ? 128 : 64;
    const int64_t grid = E * (N / 128) * (K / bko);
    TORCH_CHECK(grid < (int64_t)1 << 31, "grouped_gemm_wgrad: grid too large");
    auto stream = at::cuda::getCurrentCUDAStream();
#define LAUNCH(BKOV)                                                          \
    hipLaunchKernelGGL((grouped_wgrad_kernel<BKOV>), dim3((unsigned)grid),    \
        dim3(NTHREADS), 0, stream,                                            \
        reinterpret_cast<const bf16*>(dY.data_ptr()),                         \
        reinterpret_cast<const bf16*>(X.data_ptr()),                          \
        offsets.data_ptr<int>(), reinterpret_cast<bf16*>(dW.data_ptr()),      \
        want_bias_grad ? db.data_ptr<float>() : nullptr, (int)T, (int)E,      \
        (int)N, (int)K)
    if (bko == 128) LAUNCH(128);
    else LAUNCH(64);
#undef LAUNCH
    HIP_CHECK_LAUNCH();
    return {dW, db};
}

namespace {

// Both tables of a gated bank: E matrices of one [I,K] shape each.
void collect_glu_weights(const std::vector<torch::Tensor>& w_gate,
                         const std::vector<torch::Tensor>& w_up,
                         const torch::Tensor& like, WeightPtrs& wg,
                         WeightPtrs& wu, int64_t& I, int64_t& K) {
    int64_t Iu, Ku;
    collect_weights(w_gate, like, wg, I, K);
    collect_weights(w_up, like, wu, Iu, Ku);
    TORCH_CHECK(w_gate.size() == w_up.size() && Iu == I && Ku == K,
                "grouped_glu: gate and up banks must hold the same number "
                "of [I,K] weights");
}

}  // namespace

std::vector<torch::Tensor> grouped_glu_fwd(torch::Tensor X,
                                           std::vector<torch::Tensor> w_gate,
                                           std::vector<torch::Tensor> w_up,
                                           torch::Tensor offsets,
                                           bool save_gu) {
    check_rows(X, "X");
    WeightPtrs wg, wu;
    int64_t I, K;
    collect_glu_weights(w_gate, w_up, X, wg, wu, I, K);
    const int64_t E = (int64_t)w_gate.size(), T = X.size(0);
    TORCH_CHECK(X.size(1) == K, "grouped_glu_fwd: X is [T,", X.size(1),
                "] but weights are [", I, ",", K, "]");
    check_offsets(offsets, X, E);
    auto H = torch::empty({T, I}, X.options());
    torch::Tensor G, U;
    if (save_gu) {
        G = torch::empty({T, I}, X.options());
        U = torch::empty({T, I}, X.options());
    } else {
        G = torch::empty({0}, X.options());
        U = torch::empty({0}, X.options());
    }
    if (T == 0) return {H, G, U};
    const int64_t n_tiles_n = I / 64;
    const int64_t grid = m_tiles_bound(T, E) * n_tiles_n;
    TORCH_CHECK(grid < (int64_t)1 << 31, "grouped_glu_fwd: grid too large");
    auto stream = at::cuda::getCurrentCUDAStream();
#define LAUNCH(SAVEV)                                                         \
    hipLaunchKernelGGL((grouped_glu_fwd_kernel<SAVEV>),                       \
        dim3((unsigned)grid), dim3(NTHREADS), 0, stream,                      \
        reinterpret_cast<const bf16*>(X.data_ptr()), wg, wu,                  \
        offsets.data_ptr<int>(), reinterpret_cast<bf16*>(H.data_ptr()),       \
        reinterpret_cast<bf16*>(G.data_ptr()),                                \
        reinterpret_cast<bf16*>(U.data_ptr()), (int)T, (int)E, (int)K,        \
        (int)I, (int)n_tiles_n)
    if (save_gu) LAUNCH(true);
    else LAUNCH(false);
#undef LAUNCH
    HIP_CHECK_LAUNCH();
    return {H, G, U};
}

torch::Tensor grouped_glu_dgrad(torch::Tensor dG, torch::Tensor dU,
                                std::vector<torch::Tensor> w_gate,
                                std::vector<torch::Tensor> w_up,
                                torch::Tensor offsets) {
    check_rows(dG, "dg");
    check_rows(dU, "du");
    WeightPtrs wg, wu;
    int64_t I, K;
    collect_glu_weights(w_gate, w_up, dG, wg, wu, I, K);
    const int64_t E = (int64_t)w_gate.size(), T = dG.size(0);
    TORCH_CHECK(dU.device() == dG.device() && dG.size(1) == I &&
                    dU.size(0) == T && dU.size(1) == I,
                "grouped_glu_dgrad: dg and du must both be [T,", I,
                "] on one device");
    check_offsets(offsets, dG, E);
    auto dX = torch::empty({T, K}, dG.options());
    if (T == 0) return dX;
    // output columns run over K, which is only a multiple of 64
    const int bn = (K % 128 == 0) ? 128 : 64;
    const int64_t n_tiles_n = K / bn;
    const int64_t grid = m_tiles_bound(T, E) * n_tiles_n;
    TORCH_CHECK(grid < (int64_t)1 << 31, "grouped_glu_dgrad: grid too large");
    auto stream = at::cuda::getCurrentCUDAStream();
#define LAUNCH(BNV)                                                           \
    hipLaunchKernelGGL((grouped_glu_dgrad_kernel<BNV>),                       \
        dim3((unsigned)grid), dim3(NTHREADS), 0, stream,                      \
        reinterpret_cast<const bf16*>(dG.data_ptr()),                         \
        reinterpret_cast<const bf16*>(dU.data_ptr()), wg, wu,                 \
        offsets.data_ptr<int>(), reinterpret_cast<bf16*>(dX.data_ptr()),      \
        (int)T, (int)E, (int)I, (int)K, (int)n_tiles_n)
    if (bn == 128) LAUNCH(128);
    else LAUNCH(64);
#undef LAUNCH
    HIP_CHECK_LAUNCH();
    return dX;
}
