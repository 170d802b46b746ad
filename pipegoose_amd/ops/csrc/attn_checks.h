// Host-side operand checks shared by the decode and paged attention ops
// (decode_attention.hip, paged_prefill_attention.hip).
#pragma once

#include <torch/extension.h>

namespace attn_checks {

// a bf16 4-d device tensor of the given sizes whose rows the kernel can read
// as 16-byte packets
inline void check_operand(const char* op, const char* name,
                          const torch::Tensor& t, torch::IntArrayRef sizes) {
    TORCH_CHECK(t.is_cuda(), op, ": ", name, " must be on the GPU");
    TORCH_CHECK(t.scalar_type() == torch::kBFloat16, op, ": ", name,
                " must be bf16");
    TORCH_CHECK(t.sizes() == sizes, op, ": ", name, " has sizes ",
                t.sizes(), ", expected ", sizes);
    TORCH_CHECK(t.stride(3) == 1, op, ": last dim of ", name,
                " must be contiguous");
    for (int i = 0; i < 3; ++i)
        TORCH_CHECK(t.size(i) == 1 || t.stride(i) % 8 == 0, op, ": ",
                    name, " stride ", i, " must be a multiple of 8 elements");
    TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0,
                op, ": ", name, " must be 16-byte aligned");
}

// an int64 device tensor of 1 or B elements that a kernel reads as the
// position (decode), the first position to write (paged_kv_write) or the
// first query position (paged_prefill_attn)
inline void check_position(const char* op, const char* name,
                           const torch::Tensor& t, int64_t B) {
    TORCH_CHECK(t.is_cuda() && t.scalar_type() == torch::kLong &&
                t.is_contiguous() && (t.numel() == 1 || t.numel() == B),
                op, ": ", name, " must be a contiguous int64 GPU tensor "
                "with 1 or ", B, " elements");
}

// The two pools [n_pages, Hkv, PAGE, D] and the table [B, max_pages] of the
// paged ops; returns log2(PAGE).
inline int check_paged(const char* op, const torch::Tensor& k_pool,
                       const torch::Tensor& v_pool,
                       const torch::Tensor& block_table, int64_t B, int64_t D,
                       const torch::Device& device) {
    TORCH_CHECK(k_pool.dim() == 4 && v_pool.dim() == 4, op,
                ": k_pool and v_pool must be [n_pages, Hkv, PAGE, D]");
    const int64_t n_pages = k_pool.size(0), Hkv = k_pool.size(1);
    const int64_t page = k_pool.size(2);
    TORCH_CHECK(page == 16 || page == 32 || page == 64 || page == 128, op,
                ": page size must be 16, 32, 64 or 128, got ", page);
    TORCH_CHECK(D == 64 || D == 128, op,
                ": head dim must be 64 or 128, got ", D);
    check_operand(op, "k_pool", k_pool, {n_pages, Hkv, page, D});
    check_operand(op, "v_pool", v_pool, {n_pages, Hkv, page, D});
    TORCH_CHECK(n_pages > 0 && n_pages < (int64_t)1 << 31 && Hkv > 0, op,
                ": the pools must hold at least one page and one head");
    TORCH_CHECK(block_table.is_cuda() &&
                block_table.scalar_type() == torch::kInt, op,
                ": block_table must be an int32 GPU tensor");
    TORCH_CHECK(block_table.dim() == 2 && block_table.size(0) == B &&
                block_table.size(1) > 0 &&
                (block_table.stride(1) == 1 || block_table.size(1) == 1), op,
                ": block_table must be [", B, ", max_pages] with contiguous "
                "rows, got sizes ", block_table.sizes());
    TORCH_CHECK(block_table.size(1) * page < (int64_t)1 << 30, op,
                ": max_pages * PAGE too large");
    TORCH_CHECK(k_pool.device() == device && v_pool.device() == device &&
                block_table.device() == device, op,
                ": all operands must be on the same device");
    int shift = 4;
    while ((1 << shift) < page) ++shift;
    return shift;
}

}  // namespace attn_checks
