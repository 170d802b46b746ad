// Python bindings for the pipegoose_amd CDNA4 kernel extension.
#include <torch/extension.h>

std::vector<torch::Tensor> layer_norm_fwd(torch::Tensor x, torch::Tensor w,
                                          torch::Tensor b, double eps);
std::vector<torch::Tensor> layer_norm_bwd(torch::Tensor dy, torch::Tensor x,
                                          torch::Tensor w, torch::Tensor mean,
                                          torch::Tensor rstd);
std::vector<torch::Tensor> layer_norm_res_fwd(torch::Tensor x, torch::Tensor r,
                                              torch::Tensor w, torch::Tensor b,
                                              double eps);
torch::Tensor bias_gelu_fwd(torch::Tensor x, torch::Tensor bias);
std::vector<torch::Tensor> bias_gelu_bwd(torch::Tensor dy, torch::Tensor x,
                                         torch::Tensor bias);
std::vector<torch::Tensor> cross_entropy_fwd(torch::Tensor logits, torch::Tensor targets,
                                             int64_t vocab_start, int64_t vocab_end);
torch::Tensor cross_entropy_bwd(torch::Tensor logits, torch::Tensor targets,
                                torch::Tensor row_max, torch::Tensor row_sumexp,
                                torch::Tensor gscale, int64_t vocab_start,
                                int64_t vocab_end);
std::vector<torch::Tensor> attn_fwd(torch::Tensor q, torch::Tensor k,
                                    torch::Tensor v, torch::Tensor slopes,
                                    double scale, int64_t kv_off);
std::vector<torch::Tensor> attn_bwd(torch::Tensor dout, torch::Tensor q,
                                    torch::Tensor k, torch::Tensor v,
                                    torch::Tensor o, torch::Tensor lse,
                                    torch::Tensor slopes, double scale,
                                    int64_t kv_off);
void attn_bwd_into(torch::Tensor dout, torch::Tensor q,
                   torch::Tensor k, torch::Tensor v,
                   torch::Tensor o, torch::Tensor lse,
                   torch::Tensor slopes, double scale,
                   torch::Tensor dq, torch::Tensor dk, torch::Tensor dv,
                   int64_t kv_off);
std::tuple<std::string, int64_t> attn_variant(int64_t S, int64_t D);
torch::Tensor decode_attn(torch::Tensor q, torch::Tensor k, torch::Tensor v,
                          torch::Tensor slopes, double scale,
                          c10::optional<torch::Tensor> pos, int64_t n_splits);
std::tuple<int64_t, int64_t> decode_attn_plan(int64_t B, int64_t Hkv,
                                              int64_t Skv, int64_t D);
torch::Tensor paged_decode_attn(torch::Tensor q, torch::Tensor k_pool,
                                torch::Tensor v_pool,
                                torch::Tensor block_table,
                                torch::Tensor slopes, double scale,
                                torch::Tensor pos, int64_t n_splits);
void paged_kv_write(torch::Tensor k_new, torch::Tensor v_new,
                    torch::Tensor k_pool, torch::Tensor v_pool,
                    torch::Tensor block_table, torch::Tensor start);
torch::Tensor paged_prefill_attn(torch::Tensor q, torch::Tensor k_pool,
                                 torch::Tensor v_pool,
                                 torch::Tensor block_table,
                                 torch::Tensor slopes, double scale,
                                 torch::Tensor start);
torch::Tensor mfma_probe(torch::Tensor A, torch::Tensor Bt);
torch::Tensor mfma_probe32(torch::Tensor A, torch::Tensor Bt);
torch::Tensor tr16_probe(torch::Tensor tile);
torch::Tensor gemm_bt(torch::Tensor A, torch::Tensor B,
                      c10::optional<torch::Tensor> bias, bool gelu);
void adamw_fused_step(std::vector<torch::Tensor> params,
                      std::vector<torch::Tensor> grads,
                      std::vector<torch::Tensor> exp_avgs,
                      std::vector<torch::Tensor> exp_avg_sqs,
                      torch::Tensor meta_dev, int64_t n_slabs,
                      double lr, double beta1, double beta2, double eps,
                      double weight_decay, int64_t step);
std::vector<torch::Tensor> rms_norm_fwd(torch::Tensor x, torch::Tensor w,
                                        double eps);
std::vector<torch::Tensor> rms_norm_bwd(torch::Tensor dy, torch::Tensor x,
                                        torch::Tensor w, torch::Tensor rstd);
torch::Tensor rope_apply(torch::Tensor x, double theta_base, bool backward,
                         int64_t pos_offset);
std::vector<torch::Tensor> router_topk(torch::Tensor logits, int64_t k);
torch::Tensor silu_mul_fwd(torch::Tensor gate, torch::Tensor up);
std::vector<torch::Tensor> silu_mul_bwd(torch::Tensor dy, torch::Tensor gate,
                                        torch::Tensor up);
std::vector<torch::Tensor> fp8_quant(torch::Tensor x, bool e5m2);
std::vector<torch::Tensor> fp8_quant_dual(torch::Tensor x, bool e5m2);
torch::Tensor fp8_transpose(torch::Tensor q);
torch::Tensor grouped_gemm_fwd(torch::Tensor X,
                               std::vector<torch::Tensor> weights,
                               torch::Tensor offsets,
                               c10::optional<torch::Tensor> bias);
torch::Tensor grouped_gemm_dgrad(torch::Tensor dY,
                                 std::vector<torch::Tensor> weights,
                                 torch::Tensor offsets);
std::vector<torch::Tensor> grouped_gemm_wgrad(torch::Tensor dY,
                                              torch::Tensor X,
                                              torch::Tensor offsets,
                                              int64_t E,
                                              bool want_bias_grad);
std::vector<torch::Tensor> grouped_glu_fwd(torch::Tensor X,
                                           std::vector<torch::Tensor> w_gate,
                                           std::vector<torch::Tensor> w_up,
                                           torch::Tensor offsets,
                                           bool save_gu);
torch::Tensor grouped_glu_dgrad(torch::Tensor dG, torch::Tensor dU,
                                std::vector<torch::Tensor> w_gate,
                                std::vector<torch::Tensor> w_up,
                                torch::Tensor offsets);
std::vector<torch::Tensor> moe_route_plan(torch::Tensor order,
                                          c10::optional<torch::Tensor> weight,
                                          int64_t e0, int64_t E);
torch::Tensor moe_permute_fwd(torch::Tensor x, torch::Tensor slot_of_row,
                              int64_t k);
torch::Tensor moe_permute_bwd(torch::Tensor dxs, torch::Tensor row_of_slot,
                              int64_t N, int64_t k);
torch::Tensor moe_combine_fwd(torch::Tensor ys,
                              c10::optional<torch::Tensor> gates,
                              torch::Tensor row_of_slot, int64_t N,
                              int64_t k);
std::vector<torch::Tensor> moe_combine_bwd(torch::Tensor dout,
                                           torch::Tensor ys,
                                           c10::optional<torch::Tensor> gates,
                                           torch::Tensor slot_of_row,
                                           int64_t k, bool want_dgate);

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
    m.def("layer_norm_fwd", &layer_norm_fwd, "fused LayerNorm forward (gfx950)");
    m.def("layer_norm_bwd", &layer_norm_bwd, "fused LayerNorm backward (gfx950)");
    m.def("layer_norm_res_fwd", &layer_norm_res_fwd,
          "fused residual-add + LayerNorm forward (gfx950)");
    m.def("bias_gelu_fwd", &bias_gelu_fwd, "fused bias+GeLU forward (gfx950)");
    m.def("bias_gelu_bwd", &bias_gelu_bwd, "fused bias+GeLU backward (gfx950)");
    m.def("cross_entropy_fwd", &cross_entropy_fwd,
          "fused online-softmax CE forward over a vocab shard (gfx950)");
    m.def("cross_entropy_bwd", &cross_entropy_bwd,
          "fused CE backward: (softmax - onehot) * g (gfx950)");
    m.def("attn_fwd", &attn_fwd,
          "flash attention fwd, causal + in-kernel ALiBi (gfx950 MFMA)");
    m.def("attn_bwd", &attn_bwd,
          "flash attention bwd (two-pass, no atomics) (gfx950 MFMA)");
    m.def("attn_bwd_into", &attn_bwd_into,
          "flash attention bwd writing grads into caller buffers "
          "(e.g. fused-qkv gradient slices)");
    m.def("attn_variant", &attn_variant,
          "(S, D) -> (kernel family \"v1\"/\"v2\", waves per workgroup): the "
          "selection table attn_fwd and attn_bwd share; raises on "
          "unsupported shapes");
    m.def("decode_attn", &decode_attn,
          "single-query attention over a KV cache: split-KV, in-kernel "
          "causal + ALiBi + GQA, position read on the device (gfx950)",
          py::arg("q"), py::arg("k"), py::arg("v"), py::arg("slopes"),
          py::arg("scale"), py::arg("pos") = c10::nullopt,
          py::arg("n_splits") = 0);
    m.def("decode_attn_plan", &decode_attn_plan,
          "(B, Hkv, Skv, D) -> (n_splits, chunk): the auto split-KV plan of "
          "decode_attn; raises on unsupported shapes");
    m.def("paged_decode_attn", &paged_decode_attn,
          "decode_attn over a paged cache: pools [n_pages, Hkv, PAGE, D], "
          "int32 block_table [B, max_pages], page ids clamped in-kernel; the "
          "plan is decode_attn_plan(B, Hkv, max_pages*PAGE, D) (gfx950)",
          py::arg("q"), py::arg("k_pool"), py::arg("v_pool"),
          py::arg("block_table"), py::arg("slopes"), py::arg("scale"),
          py::arg("pos"), py::arg("n_splits") = 0);
    m.def("paged_kv_write", &paged_kv_write,
          "write new K/V rows [B, Hkv, S_new, D] into the paged pools at "
          "logical positions start[b] + s (start read on the device); rows "
          "past max_pages*PAGE are dropped (gfx950)",
          py::arg("k_new"), py::arg("v_new"), py::arg("k_pool"),
          py::arg("v_pool"), py::arg("block_table"), py::arg("start"));
    m.def("paged_prefill_attn", &paged_prefill_attn,
          "causal attention of Sq >= 1 query rows at positions start[b] + i "
          "over a paged cache (chunked prefill, prefix reuse): start read on "
          "the device, page ids clamped in-kernel, rows outside "
          "[0, max_pages*PAGE) give zeros (gfx950 MFMA)",
          py::arg("q"), py::arg("k_pool"), py::arg("v_pool"),
          py::arg("block_table"), py::arg("slopes"), py::arg("scale"),
          py::arg("start"));
    m.def("mfma_probe", &mfma_probe,
          "16x16x32 bf16 MFMA fragment-layout probe");
    m.def("mfma_probe32", &mfma_probe32,
          "32x32x16 bf16 MFMA fragment-layout probe");
    m.def("tr16_probe", &tr16_probe,
          "ds_read_b64_tr_b16 semantics probe ([4][16] tile -> per-lane)");
    m.def("gemm_bt", &gemm_bt,
          "hand-written MFMA bf16 GEMM C = A @ B^T (+bias, +gelu) (gfx950)",
          py::arg("A"), py::arg("B"), py::arg("bias") = c10::nullopt,
          py::arg("gelu") = false);
    m.def("adamw_fused_step", &adamw_fused_step,
          "whole AdamW update, one chunked kernel per step (gfx950)");
    m.def("rms_norm_fwd", &rms_norm_fwd, "fused RMSNorm forward (gfx950)");
    m.def("rms_norm_bwd", &rms_norm_bwd, "fused RMSNorm backward (gfx950)");
    m.def("rope_apply", &rope_apply,
          "rotary embedding with in-kernel cos/sin (gfx950)");
    m.def("router_topk", &router_topk,
          "fused Switch router: softmax+topk+colsum+lse in one pass (gfx950)");
    m.def("fp8_quant", &fp8_quant,
          "dynamic per-tensor fp8 quantize: one amax pass + one cast pass");
    m.def("fp8_quant_dual", &fp8_quant_dual,
          "fp8 quantize emitting row-major AND transposed images in one "
          "read (kills the separate backward-layout transpose pass)");
    m.def("fp8_transpose", &fp8_transpose,
          "LDS-tiled byte transpose for fp8 GEMM operand layouts");
    m.def("silu_mul_fwd", &silu_mul_fwd, "fused SwiGLU silu(g)*u (gfx950)");
    m.def("silu_mul_bwd", &silu_mul_bwd, "fused SwiGLU backward (gfx950)");
    m.def("grouped_gemm_fwd", &grouped_gemm_fwd,
          "grouped expert GEMM Y[r] = X[r] @ W[e]^T (+b[e]) over an "
          "expert-sorted ragged buffer (gfx950 MFMA)",
          py::arg("X"), py::arg("weights"), py::arg("offsets"),
          py::arg("bias") = c10::nullopt);
    m.def("grouped_gemm_dgrad", &grouped_gemm_dgrad,
          "grouped expert GEMM input grad dX[r] = dY[r] @ W[e] (gfx950 MFMA)");
    m.def("grouped_gemm_wgrad", &grouped_gemm_wgrad,
          "grouped expert GEMM weight/bias grads, deterministic: "
          "dW[e] = dY_e^T @ X_e, db[e] = colsum(dY_e) (gfx950 MFMA)");
    m.def("grouped_glu_fwd", &grouped_glu_fwd,
          "gated expert bank forward: g = X @ Wg[e]^T, u = X @ Wu[e]^T and "
          "h = silu(g) * u from one read of X -> (h, g, u) (gfx950 MFMA)",
          py::arg("X"), py::arg("w_gate"), py::arg("w_up"),
          py::arg("offsets"), py::arg("save_gu") = true);
    m.def("grouped_glu_dgrad", &grouped_glu_dgrad,
          "gated expert bank input grad dX[r] = dg[r] @ Wg[e] + du[r] @ "
          "Wu[e], one fp32 accumulator, one rounding (gfx950 MFMA)");
    m.def("moe_route_plan", &moe_route_plan,
          "MoE routing plan: stable counting sort of the kept slots by "
          "local expert -> (offsets, row_of_slot, slot_of_row); no host "
          "sync, no atomics (gfx950)");
    m.def("moe_permute_fwd", &moe_permute_fwd,
          "gather token rows into the expert-sorted buffer (gfx950)");
    m.def("moe_permute_bwd", &moe_permute_bwd,
          "sum a token's expert-sorted grad rows, fp32, no atomics (gfx950)");
    m.def("moe_combine_fwd", &moe_combine_fwd,
          "gate-weighted sum of a token's expert output rows (gfx950)");
    m.def("moe_combine_bwd", &moe_combine_bwd,
          "combine backward: dys and dgate from one read of dout (gfx950)");
}
