// Decode ("flash-decoding") attention for gfx950: ONE query row per batch row
// and q head against a static KV cache, causal up to a device-side position,
// with the ALiBi bias and the GQA head mapping computed in-kernel.
//
//   o[b,h,:] = softmax_j( scale * q[b,h,:]·k[b,h/G,j,:] + slopes[h]*(j-p) )
//              @ v[b,h/G,j,:]          j in [0, p] inclusive, p = pos[b]
//
// q [B,H,1,D], k/v [B,Hkv,Skv,D] bf16, any batch/head/row strides (d
// contiguous, 16-byte aligned rows); D in {64,128}; G = H/Hkv; Skv >= 1, no
// divisibility requirement.  p is READ ON THE DEVICE from `pos` (int64, 1 or B
// elements), so a captured hipGraph replays with the position as data; with
// no `pos` the host passes p = Skv-1 as a scalar.  0 <= p < Skv is a
// precondition; the kernels clamp p into that range and clamp every row index
// to p, so nothing past p is ever even loaded: slots j > p may hold ANY bits.
//
// Split-KV, two plain launches, no atomics, no inter-workgroup hand-off:
//
//   decode_attn_split_kernel   grid (n_splits, Hkv, B), 4 waves.  Split s owns
//       keys [s*chunk, (s+1)*chunk); a split that starts beyond p exits at
//       once.  The workgroup serves all G q heads of its kv head (K/V leave
//       HBM once per group) and writes, per q head, an fp32 partial
//       (m, l, acc[D]) in the exp2 domain to a workspace.
//   decode_attn_combine_kernel grid (H, B), D threads.  Merges the partials of
//       the LIVE splits (s*chunk <= p; each holds at least one key, so l > 0
//       and no (-inf)-(-inf) or 0/0 can arise) in split order and writes bf16.
//
// K/V go straight from HBM to VGPRs as 16-byte-per-lane loads (no LDS round
// trip: nothing is shared between waves).  D/8 lanes hold one row, so a wave
// load covers 64/(D/8) consecutive rows; q·k is a DPP butterfly over those
// D/8 lanes (no LDS traffic).  Each lane group keeps its OWN online-softmax state (m, l, acc) for
// the rows it sees; the states merge once at the end (across lane groups by
// shuffles, across waves through LDS), always in the same order: results are
// bit-reproducible for fixed inputs and plan.
//
// The plan depends only on host-known shapes, never on p (static grid under
// graph capture).  TILE = 64 keys per workgroup iteration.
//
//   auto (n_splits = 0):  n = ceil(1024 / (B*Hkv)) workgroups' worth,
//                         clamped to [1, min(MAX_SPLITS, ceil(Skv/TILE))];
//                         chunk = round_up(ceil(Skv/n), TILE);
//                         n_splits = ceil(Skv/chunk)      (no empty splits)
//   forced n_splits in [1, MAX_SPLITS = 64]:
//                         chunk = round_up(ceil(Skv/n_splits), TILE);
//                         n_splits stays as given (trailing splits may be
//                         empty and exit at once)
//
// decode_attn_plan(B, Hkv, Skv, D) returns the auto (n_splits, chunk).
//
// PAGED caches (paged_decode_attn): the same split kernel with PAGED = true.
// K and V live in pools [n_pages, Hkv, PAGE, D] shared by all sequences, and
// logical key row j of batch row b is
//
//   pool[clamp(block_table[b, j / PAGE], 0, n_pages-1), h/G, j % PAGE, :]
//
// with block_table int32 [B, max_pages] (row stride free) and PAGE a power of
// two in {16, 32, 64, 128}.  Skv := max_pages * PAGE, the plan is make_plan on
// that, pos is required.  TILE = 64 and NW = 4 give each wave 16 consecutive,
// 16-aligned rows per tile, and the clamp of a row index to p stays inside
// them (the wave is only there when its first row is <= p), so for every
// allowed PAGE the rows a wave loads in one tile sit in ONE page: the table
// lookup is wave-uniform, one int32 per wave per tile, made uniform with
// readfirstlane so that it is a scalar load held in an SGPR.  It adds no
// per-lane load to the K/V address path; the id of the next tile is fetched
// while the current tile is computed.  "Nothing beyond p is loaded" extends
// to the table: entries with index > p / PAGE are never read.  Every id that
// is read is clamped into [0, n_pages-1] before use, so a corrupt table gives
// wrong numbers and never an out-of-bounds access.  The contiguous
// instantiations (PAGED = false) compile the address path they always had.
// The combine kernel is shared as is.
//
// paged_kv_write(k_new, v_new, k_pool, v_pool, block_table, start): one
// launch, one thread per 16-byte packet of a new row, K and V both.  Row s of
// batch row b ([B, Hkv, S_new, D], any strides with d contiguous) goes to
// logical position start[b] + s through the table with the same id clamp;
// `start` (int64, 1 or B elements) is READ ON THE DEVICE, so the call is
// graph-capturable with the position as data.  For the same reason
// start + S_new <= max_pages * PAGE cannot be checked on the host: rows whose
// logical position is < 0 or >= max_pages * PAGE are DROPPED (no wrap, no
// overrun, no table read).  Nothing but the addressed rows is written.
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

#include <cfloat>
#include <tuple>
#include <type_traits>

#include "attn_checks.h"
#include "common.h"

namespace {

using bf16 = __hip_bfloat16;
using attn_checks::check_operand;
using attn_checks::check_paged;
using attn_checks::check_position;

constexpr int TILE = 64;        // keys per workgroup iteration
constexpr int NW = 4;           // waves per workgroup
constexpr int MAX_SPLITS = 64;
constexpr int TARGET_WGS = 1024;
constexpr float LOG2E = 1.4426950408889634f;

__device__ __forceinline__ float bf16_lo(uint32_t w) {
    return __uint_as_float(w << 16);
}
__device__ __forceinline__ float bf16_hi(uint32_t w) {
    return __uint_as_float(w & 0xffff0000u);
}
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
    return x + __int_as_float(__builtin_amdgcn_update_dpp(
                   0, __float_as_int(x), CTRL, 0xf, 0xf, true));
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

// GT q heads of the group are processed per pass over the split's keys
// (GT = 4, 2 or 1, the largest that divides G); G > 4 takes G/GT passes, the
// later ones reading the chunk from cache.
//
// PAGED: k and v are the page pools, kb/vb the page strides, and rows are
// addressed through block_table (file header); otherwise the four paged
// arguments are unused.
template <int D, int GT, bool PAGED>
__global__ __launch_bounds__(NW * WAVE_SIZE)
void decode_attn_split_kernel(const bf16* __restrict__ q,
                              const bf16* __restrict__ k,
                              const bf16* __restrict__ v,
                              const float* __restrict__ slopes, float scale,
                              const int64_t* __restrict__ pos, int pos_n,
                              int pos_scalar,
                              float* __restrict__ part_acc,  // [B,H,n_splits,D]
                              float* __restrict__ part_ml,   // [B,H,n_splits,2]
                              int H, int G, int Skv, int chunk, int n_splits,
                              int64_t qb, int64_t qh,
                              int64_t kb, int64_t kh, int64_t ks,
                              int64_t vb, int64_t vh, int64_t vs,
                              const int* __restrict__ block_table,
                              int64_t bt_stride, int n_pages, int page_shift) {
    constexpr int TPR = D / 8;             // lanes per row
    constexpr int RPW = WAVE_SIZE / TPR;   // rows per wave load
    constexpr int RW = TILE / NW;          // rows per wave per tile
    constexpr int NL = RW / RPW;           // loads per wave per tile (K, and V)

    __shared__ float s_acc[NW][GT][D];
    __shared__ float s_ml[NW][GT][2];

    const int split = blockIdx.x;
    const int hk = blockIdx.y;
    const int b = blockIdx.z;
    const int p = load_pos(pos, pos_n, pos_scalar, b, Skv);
    const int c0 = split * chunk;
    if (c0 > p) return;                    // split wholly beyond p: no partial
    const int end = min(c0 + chunk, p + 1);

    const int tid = threadIdx.x;
    const int wave = tid / WAVE_SIZE;
    const int lane = tid % WAVE_SIZE;
    const int sub = lane % TPR;            // which 8 of the D columns
    const int slot = lane / TPR;           // which row of a wave load

    const bf16* kp = k + (PAGED ? 0 : b * kb) + hk * kh + sub * 8;
    const bf16* vp = v + (PAGED ? 0 : b * vb) + hk * vh + sub * 8;
    // PAGED: this wave's rows of a tile are [tile0 + wrow, tile0 + wrow + RW),
    // inside one page; page_of reads and clamps that page's id (wave-uniform)
    static_assert(!PAGED || TILE / NW == 16, "a wave's rows must fit a page");
    const int* bt_row = PAGED ? block_table + b * bt_stride : nullptr;
    const int wrow = PAGED ? __builtin_amdgcn_readfirstlane(wave * RW) : 0;
    auto page_of = [&](int row) {
        const int id = bt_row[__builtin_amdgcn_readfirstlane(row) >> page_shift];
        return min(max(id, 0), n_pages - 1);
    };

    for (int g0 = 0; g0 < G; g0 += GT) {
        const int h0 = hk * G + g0;
        float qf[GT][8], slope2[GT];
        float m[GT], l[GT], acc[GT][8];
#pragma unroll
        for (int g = 0; g < GT; ++g) {
            const uint4 qr = *reinterpret_cast<const uint4*>(
                q + b * qb + (h0 + g) * qh + sub * 8);
            unpack8(qr, qf[g]);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                qf[g][e] *= scale * LOG2E;   // exp2 domain
                acc[g][e] = 0.f;
            }
            slope2[g] = slopes[h0 + g] * LOG2E;
            m[g] = -FLT_MAX;
            l[g] = 0.f;
        }

        int page = 0;
        if constexpr (PAGED)
            if (c0 + wrow <= p) page = page_of(c0 + wrow);
        for (int tile0 = c0; tile0 < end; tile0 += TILE) {
            const int rbase = tile0 + wave * RW;
            if (rbase > p) break;          // wave-uniform: whole tile part masked
            uint4 kr[NL], vr[NL];
#pragma unroll
            for (int i = 0; i < NL; ++i) {
                // rows past p are never loaded: the index is clamped to p
                const int rc = min(rbase + i * RPW + slot, p);
                if constexpr (PAGED) {
                    const int in_page = rc & ((1 << page_shift) - 1);
                    kr[i] = *reinterpret_cast<const uint4*>(
                        kp + page * kb + (int64_t)in_page * ks);
                    vr[i] = *reinterpret_cast<const uint4*>(
                        vp + page * vb + (int64_t)in_page * vs);
                } else {
                    kr[i] = *reinterpret_cast<const uint4*>(
                        kp + (int64_t)rc * ks);
                    vr[i] = *reinterpret_cast<const uint4*>(
                        vp + (int64_t)rc * vs);
                }
            }
            if constexpr (PAGED) {
                // the next tile's id, only if this wave will be there: table
                // entries past p / PAGE are never read
                const int nxt = tile0 + TILE + wrow;
                if (tile0 + TILE < end && nxt <= p) page = page_of(nxt);
            }
#pragma unroll
            for (int i = 0; i < NL; ++i) {
                const int r = rbase + i * RPW + slot;
                const bool valid = r <= p;
                const float rel = (float)(r - p);
                float kf[8], vf[8];
                unpack8(kr[i], kf);
                unpack8(vr[i], vf);
#pragma unroll
                for (int g = 0; g < GT; ++g) {
                    float s = 0.f;
#pragma unroll
                    for (int e = 0; e < 8; ++e) s = fmaf(qf[g][e], kf[e], s);
                    s = fmaf(slope2[g], rel, group_sum<TPR>(s));
                    // masking is a select, on the score and on the weight: a
                    // masked lane has alpha = 1 and pw = 0, and the row it
                    // holds is row p itself (the clamp above), never one from
                    // the tail, so its state stays exactly as it was
                    const float mn = valid ? fmaxf(m[g], s) : m[g];
                    const float alpha = __builtin_amdgcn_exp2f(m[g] - mn);
                    const float pw =
                        valid ? __builtin_amdgcn_exp2f(s - mn) : 0.f;
                    m[g] = mn;
                    l[g] = fmaf(l[g], alpha, pw);
#pragma unroll
                    for (int e = 0; e < 8; ++e)
                        acc[g][e] = fmaf(acc[g][e], alpha, pw * vf[e]);
                }
            }
        }

        // merge the wave's RPW lane-group states (fixed butterfly order)
#pragma unroll
        for (int g = 0; g < GT; ++g) {
#pragma unroll
            for (int off = TPR; off < WAVE_SIZE; off <<= 1) {
                const float m2 = __shfl_xor(m[g], off, WAVE_SIZE);
                const float l2 = __shfl_xor(l[g], off, WAVE_SIZE);
                float a2[8];
#pragma unroll
                for (int e = 0; e < 8; ++e)
                    a2[e] = __shfl_xor(acc[g][e], off, WAVE_SIZE);
                merge_state(m[g], l[g], acc[g], m2, l2, a2);
            }
            if (slot == 0) {
#pragma unroll
                for (int e = 0; e < 8; ++e)
                    s_acc[wave][g][sub * 8 + e] = acc[g][e];
                if (sub == 0) {
                    s_ml[wave][g][0] = m[g];
                    s_ml[wave][g][1] = l[g];
                }
            }
        }
        __syncthreads();
        // merge the NW waves in wave order, one thread per (head, column)
        for (int idx = tid; idx < GT * D; idx += NW * WAVE_SIZE) {
            const int g = idx / D, d = idx % D;
            float mm = s_ml[0][g][0], ll = s_ml[0][g][1];
            float aa[1] = {s_acc[0][g][d]};
#pragma unroll
            for (int w = 1; w < NW; ++w) {
                const float a2[1] = {s_acc[w][g][d]};
                merge_state(mm, ll, aa, s_ml[w][g][0], s_ml[w][g][1], a2);
            }
            const int64_t row =
                ((int64_t)b * H + (h0 + g)) * n_splits + split;
            part_acc[row * D + d] = aa[0];
            if (d == 0) {
                part_ml[row * 2 + 0] = mm;
                part_ml[row * 2 + 1] = ll;
            }
        }
        __syncthreads();                   // s_acc is reused by the next pass
    }
}

template <int D>
__global__ __launch_bounds__(D)
void decode_attn_combine_kernel(const float* __restrict__ part_acc,
                                const float* __restrict__ part_ml,
                                const int64_t* __restrict__ pos, int pos_n,
                                int pos_scalar,
                                bf16* __restrict__ o,        // [B,1,H,D]
                                int H, int Skv, int chunk, int n_splits) {
    const int h = blockIdx.x;
    const int b = blockIdx.y;
    const int d = threadIdx.x;
    const int p = load_pos(pos, pos_n, pos_scalar, b, Skv);
    // live splits are exactly those that start at or before p
    const int n_live = min(n_splits, p / chunk + 1);
    const int64_t row0 = ((int64_t)b * H + h) * n_splits;

    float mx = -FLT_MAX;
    for (int s = 0; s < n_live; ++s)
        mx = fmaxf(mx, part_ml[(row0 + s) * 2]);
    float num = 0.f, den = 0.f;
    for (int s = 0; s < n_live; ++s) {
        const float w = __builtin_amdgcn_exp2f(part_ml[(row0 + s) * 2] - mx);
        den = fmaf(part_ml[(row0 + s) * 2 + 1], w, den);
        num = fmaf(part_acc[(row0 + s) * D + d], w, num);
    }
    o[((int64_t)b * H + h) * D + d] = __float2bfloat16(num / den);
}

struct DecodePlan {
    int n_splits, chunk;
};

int round_up(int64_t x, int64_t to) { return (int)((x + to - 1) / to * to); }

// The plan of the file header: shapes only, never the position.
DecodePlan make_plan(int64_t B, int64_t Hkv, int64_t Skv, int64_t D,
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

// One thread per 16-byte packet of a new row; K and V in the same launch.
// Rows whose logical position falls outside [0, capacity) are dropped.
template <int D>
__global__ __launch_bounds__(256)
void paged_kv_write_kernel(const bf16* __restrict__ k_new,
                           const bf16* __restrict__ v_new,
                           bf16* __restrict__ k_pool,
                           bf16* __restrict__ v_pool,
                           const int* __restrict__ block_table,
                           int64_t bt_stride,
                           const int64_t* __restrict__ start, int start_n,
                           int64_t total, int Hkv, int S_new, int capacity,
                           int n_pages, int page_shift,
                           int64_t knb, int64_t knh, int64_t kns,
                           int64_t vnb, int64_t vnh, int64_t vns,
                           int64_t kpp, int64_t kph, int64_t kps,
                           int64_t vpp, int64_t vph, int64_t vps) {
    constexpr int TPR = D / 8;
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int sub = (int)(idx % TPR);
    int64_t rest = idx / TPR;
    const int hk = (int)(rest % Hkv);      // heads innermost: the models'
    rest /= Hkv;                           // views are [B, S, Hkv, D] in memory
    const int s = (int)(rest % S_new);
    const int b = (int)(rest / S_new);
    const int64_t row = start[start_n == 1 ? 0 : b] + s;
    if (row < 0 || row >= capacity) return;
    const int r = (int)row;
    int page = block_table[b * bt_stride + (r >> page_shift)];
    page = min(max(page, 0), n_pages - 1);
    const int in_page = r & ((1 << page_shift) - 1);
    const uint4 kv = *reinterpret_cast<const uint4*>(
        k_new + b * knb + hk * knh + s * kns + sub * 8);
    const uint4 vv = *reinterpret_cast<const uint4*>(
        v_new + b * vnb + hk * vnh + s * vns + sub * 8);
    *reinterpret_cast<uint4*>(
        k_pool + page * kpp + hk * kph + in_page * kps + sub * 8) = kv;
    *reinterpret_cast<uint4*>(
        v_pool + page * vpp + hk * vph + in_page * vps + sub * 8) = vv;
}

// The two launches behind decode_attn and paged_decode_attn.  PAGED: k and v
// are the pools and Skv = max_pages * PAGE.
template <bool PAGED>
torch::Tensor launch_decode(const torch::Tensor& q, const torch::Tensor& k,
                            const torch::Tensor& v,
                            const torch::Tensor& slopes, double scale,
                            const int64_t* pos_ptr, int pos_n,
                            const DecodePlan& plan, int64_t Hkv, int64_t Skv,
                            const int* bt_ptr, int64_t bt_stride, int n_pages,
                            int page_shift) {
    const int64_t B = q.size(0), H = q.size(1), D = q.size(3);
    const int G = (int)(H / Hkv);

    // physically [B, 1, H, D]: the model's reshape to [B, 1, H*D] is free
    auto o_phys = torch::empty({B, 1, H, D}, q.options());
    auto fopt = q.options().dtype(torch::kFloat);
    auto part_acc = torch::empty({B, H, plan.n_splits, D}, fopt);
    auto part_ml = torch::empty({B, H, plan.n_splits, 2}, fopt);

    auto stream = at::cuda::getCurrentCUDAStream();
    auto launch_split = [&](auto dv_, auto gt_) {
        constexpr int DV = decltype(dv_)::value, GT = decltype(gt_)::value;
        hipLaunchKernelGGL((decode_attn_split_kernel<DV, GT, PAGED>),
                           dim3(plan.n_splits, Hkv, B), dim3(NW * WAVE_SIZE),
                           0, stream,
                           reinterpret_cast<const bf16*>(q.data_ptr()),
                           reinterpret_cast<const bf16*>(k.data_ptr()),
                           reinterpret_cast<const bf16*>(v.data_ptr()),
                           slopes.data_ptr<float>(), (float)scale, pos_ptr,
                           pos_n, (int)(Skv - 1), part_acc.data_ptr<float>(),
                           part_ml.data_ptr<float>(), (int)H, G, (int)Skv,
                           plan.chunk, plan.n_splits,
                           q.stride(0), q.stride(1),
                           k.stride(0), k.stride(1), k.stride(2),
                           v.stride(0), v.stride(1), v.stride(2),
                           bt_ptr, bt_stride, n_pages, page_shift);
    };
    auto with_gt = [&](auto dv_) {
        if (G % 4 == 0) launch_split(dv_, std::integral_constant<int, 4>{});
        else if (G % 2 == 0) launch_split(dv_, std::integral_constant<int, 2>{});
        else launch_split(dv_, std::integral_constant<int, 1>{});
    };
    if (D == 64) with_gt(std::integral_constant<int, 64>{});
    else with_gt(std::integral_constant<int, 128>{});
    HIP_CHECK_LAUNCH();

    auto launch_combine = [&](auto dv_) {
        constexpr int DV = decltype(dv_)::value;
        hipLaunchKernelGGL((decode_attn_combine_kernel<DV>), dim3(H, B),
                           dim3(DV), 0, stream, part_acc.data_ptr<float>(),
                           part_ml.data_ptr<float>(), pos_ptr, pos_n,
                           (int)(Skv - 1),
                           reinterpret_cast<bf16*>(o_phys.data_ptr()), (int)H,
                           (int)Skv, plan.chunk, plan.n_splits);
    };
    if (D == 64) launch_combine(std::integral_constant<int, 64>{});
    else launch_combine(std::integral_constant<int, 128>{});
    HIP_CHECK_LAUNCH();
    return o_phys.permute({0, 2, 1, 3});
}

}  // namespace

std::tuple<int64_t, int64_t> decode_attn_plan(int64_t B, int64_t Hkv,
                                              int64_t Skv, int64_t D) {
    const DecodePlan plan = make_plan(B, Hkv, Skv, D, 0);
    return {plan.n_splits, plan.chunk};
}


torch::Tensor decode_attn(torch::Tensor q, torch::Tensor k, torch::Tensor v,
                          torch::Tensor slopes, double scale,
                          c10::optional<torch::Tensor> pos, int64_t n_splits) {
    TORCH_CHECK(q.dim() == 4 && k.dim() == 4 && v.dim() == 4,
                "decode_attn: q must be [B, H, 1, D], k and v [B, Hkv, Skv, D]");
    const int64_t B = q.size(0), H = q.size(1), D = q.size(3);
    const int64_t Hkv = k.size(1), Skv = k.size(2);
    check_operand("decode_attn", "q", q, {B, H, 1, D});
    check_operand("decode_attn", "k", k, {B, Hkv, Skv, D});
    check_operand("decode_attn", "v", v, {B, Hkv, Skv, D});
    TORCH_CHECK(Hkv > 0 && H % Hkv == 0,
                "decode_attn: q heads must be a multiple of kv heads");
    TORCH_CHECK(k.device() == q.device() && v.device() == q.device(),
                "decode_attn: q, k and v must be on the same device");
    TORCH_CHECK(slopes.is_cuda() && slopes.scalar_type() == torch::kFloat &&
                slopes.numel() == H && slopes.is_contiguous(),
                "decode_attn: slopes must be ", H,
                " contiguous fp32 values on the GPU");
    const int64_t* pos_ptr = nullptr;
    int pos_n = 0;
    if (pos.has_value()) {
        check_position("decode_attn", "pos", *pos, B);
        pos_ptr = pos->data_ptr<int64_t>();
        pos_n = (int)pos->numel();
    }
    const DecodePlan plan = make_plan(B, Hkv, Skv, D, n_splits);
    TORCH_CHECK(Hkv <= 65535 && B <= 65535 && H <= 65535,
                "decode_attn: B, H and Hkv must fit a grid dimension");
    return launch_decode<false>(q, k, v, slopes, scale, pos_ptr, pos_n, plan,
                                Hkv, Skv, nullptr, 0, 0, 0);
}

torch::Tensor paged_decode_attn(torch::Tensor q, torch::Tensor k_pool,
                                torch::Tensor v_pool,
                                torch::Tensor block_table,
                                torch::Tensor slopes, double scale,
                                torch::Tensor pos, int64_t n_splits) {
    const char* op = "paged_decode_attn";
    TORCH_CHECK(q.dim() == 4, op, ": q must be [B, H, 1, D]");
    const int64_t B = q.size(0), H = q.size(1), D = q.size(3);
    check_operand(op, "q", q, {B, H, 1, D});
    const int shift = check_paged(op, k_pool, v_pool, block_table, B, D,
                                  q.device());
    const int64_t n_pages = k_pool.size(0), Hkv = k_pool.size(1);
    const int64_t Skv = block_table.size(1) << shift;
    TORCH_CHECK(H % Hkv == 0, op,
                ": q heads must be a multiple of kv heads");
    TORCH_CHECK(slopes.is_cuda() && slopes.scalar_type() == torch::kFloat &&
                slopes.numel() == H && slopes.is_contiguous(), op,
                ": slopes must be ", H, " contiguous fp32 values on the GPU");
    check_position(op, "pos", pos, B);
    const DecodePlan plan = make_plan(B, Hkv, Skv, D, n_splits);
    TORCH_CHECK(Hkv <= 65535 && B <= 65535 && H <= 65535, op,
                ": B, H and Hkv must fit a grid dimension");
    return launch_decode<true>(q, k_pool, v_pool, slopes, scale,
                               pos.data_ptr<int64_t>(), (int)pos.numel(),
                               plan, Hkv, Skv, block_table.data_ptr<int>(),
                               block_table.stride(0), (int)n_pages, shift);
}

void paged_kv_write(torch::Tensor k_new, torch::Tensor v_new,
                    torch::Tensor k_pool, torch::Tensor v_pool,
                    torch::Tensor block_table, torch::Tensor start) {
    const char* op = "paged_kv_write";
    TORCH_CHECK(k_new.dim() == 4 && v_new.dim() == 4, op,
                ": k_new and v_new must be [B, Hkv, S_new, D]");
    const int64_t B = k_new.size(0), Hkv = k_new.size(1);
    const int64_t S_new = k_new.size(2), D = k_new.size(3);
    check_operand(op, "k_new", k_new, {B, Hkv, S_new, D});
    check_operand(op, "v_new", v_new, {B, Hkv, S_new, D});
    const int shift = check_paged(op, k_pool, v_pool, block_table, B, D,
                                  k_new.device());
    TORCH_CHECK(v_new.device() == k_new.device(), op,
                ": all operands must be on the same device");
    TORCH_CHECK(k_pool.size(1) == Hkv, op, ": the pools have ",
                k_pool.size(1), " kv heads, the new rows ", Hkv);
    check_position(op, "start", start, B);
    TORCH_CHECK(S_new < (int64_t)1 << 30 && Hkv <= 65535, op,
                ": S_new or Hkv too large");
    const int64_t total = B * Hkv * S_new * (D / 8);
    if (total == 0) return;
    const int64_t capacity = block_table.size(1) << shift;
    constexpr int THREADS = 256;
    const int64_t blocks = (total + THREADS - 1) / THREADS;
    TORCH_CHECK(blocks < (int64_t)1 << 31, op, ": too many rows for one launch");

    auto stream = at::cuda::getCurrentCUDAStream();
    auto launch = [&](auto dv_) {
        constexpr int DV = decltype(dv_)::value;
        hipLaunchKernelGGL((paged_kv_write_kernel<DV>), dim3((unsigned)blocks),
                           dim3(THREADS), 0, stream,
                           reinterpret_cast<const bf16*>(k_new.data_ptr()),
                           reinterpret_cast<const bf16*>(v_new.data_ptr()),
                           reinterpret_cast<bf16*>(k_pool.data_ptr()),
                           reinterpret_cast<bf16*>(v_pool.data_ptr()),
                           block_table.data_ptr<int>(), block_table.stride(0),
                           start.data_ptr<int64_t>(), (int)start.numel(),
                           total, (int)Hkv, (int)S_new, (int)capacity,
                           (int)k_pool.size(0), shift,
                           k_new.stride(0), k_new.stride(1), k_new.stride(2),
                           v_new.stride(0), v_new.stride(1), v_new.stride(2),
                           k_pool.stride(0), k_pool.stride(1), k_pool.stride(2),
                           v_pool.stride(0), v_pool.stride(1), v_pool.stride(2));
    };
    if (D == 64) launch(std::integral_constant<int, 64>{});
    else launch(std::integral_constant<int, 128>{});
    HIP_CHECK_LAUNCH();
}
