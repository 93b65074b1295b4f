// Python bindings for the ravnest_amd CDNA4 kernel library (_C).
#include <torch/extension.h>

#include <vector>

std::vector<at::Tensor> layernorm_fwd(at::Tensor x, at::Tensor w,
                                      at::Tensor b, double eps);
std::vector<at::Tensor> layernorm_bwd(at::Tensor dy, at::Tensor x,
                                      at::Tensor w, at::Tensor mean,
                                      at::Tensor rstd);
std::vector<at::Tensor> layernorm_add_fwd(at::Tensor a, at::Tensor b,
                                          at::Tensor w, at::Tensor bias,
                                          double eps);
std::vector<at::Tensor> layernorm_mx_fwd(at::Tensor x, at::Tensor w,
                                         at::Tensor b, double eps);
at::Tensor bias_gelu_fwd(at::Tensor x, at::Tensor bias);
std::vector<at::Tensor> bias_gelu_mx_fwd(at::Tensor x, at::Tensor bias);
at::Tensor bias_gelu_bwd(at::Tensor dy, at::Tensor x, at::Tensor bias);
at::Tensor colsum_bf16(at::Tensor x);
std::vector<at::Tensor> bias_gelu_bwd_db(at::Tensor dy, at::Tensor x,
                                         at::Tensor bias);
std::vector<at::Tensor> batchnorm_fwd(at::Tensor x, at::Tensor w,
                                      at::Tensor b, at::Tensor running_mean,
                                      at::Tensor running_var, bool training,
                                      double momentum, double eps);
std::vector<at::Tensor> batchnorm_bwd(at::Tensor dy, at::Tensor x,
                                      at::Tensor w, at::Tensor mean,
                                      at::Tensor rstd, bool training);
std::vector<int64_t> batchnorm_relu_launch_constants();
std::vector<at::Tensor> batchnorm_relu_fwd(
    at::Tensor x, c10::optional<at::Tensor> residual, at::Tensor w,
    at::Tensor b, at::Tensor running_mean, at::Tensor running_var,
    bool training, double momentum, double eps);
std::vector<at::Tensor> batchnorm_relu_bwd(at::Tensor dy, at::Tensor x,
                                           at::Tensor y, at::Tensor w,
                                           at::Tensor mean, at::Tensor rstd,
                                           bool training, bool want_dr);
at::Tensor conv2d_fwd(at::Tensor x, at::Tensor w,
                      c10::optional<at::Tensor> bias, long st, long pad,
                      bool relu);
at::Tensor conv2d_dgrad(at::Tensor dy, at::Tensor w, long N, long H,
                        long W, long st, long pad);
at::Tensor conv2d_wgrad(at::Tensor dy, at::Tensor x, long R, long S,
                        long st, long pad);
std::vector<at::Tensor> mx_quant(at::Tensor x);
std::vector<at::Tensor> gemm_nt_bf16(at::Tensor A2, at::Tensor B,
                                     c10::optional<at::Tensor> bias,
                                     int64_t epi);
at::Tensor gemm_wgrad_bf16(at::Tensor dy, at::Tensor x);
void gemm_nt_bf16_rows(at::Tensor A2, at::Tensor B,
                       c10::optional<at::Tensor> bias, int64_t epi,
                       at::Tensor C, at::Tensor row_limit);
at::Tensor gemm_wgrad_bf16_rows(at::Tensor dy, at::Tensor x,
                                at::Tensor row_bound);
at::Tensor mx_gemm(at::Tensor x, at::Tensor xs, at::Tensor w,
                   at::Tensor ws, c10::optional<at::Tensor> bias);
at::Tensor mx_gemm2(at::Tensor xq, at::Tensor xs, at::Tensor wq,
                    at::Tensor ws, c10::optional<at::Tensor> bias);
at::Tensor mx_scale_probe(at::Tensor a, at::Tensor b, at::Tensor sa,
                          at::Tensor sb);
at::Tensor softmax_fwd(at::Tensor x);
at::Tensor softmax_bwd(at::Tensor dy, at::Tensor y);
std::vector<at::Tensor> maxpool2d_fwd(at::Tensor x, long K, long S, long P);
at::Tensor maxpool2d_bwd(at::Tensor dy, at::Tensor idx, long H, long W,
                         long K, long S, long P);
at::Tensor avgpool2d_fwd(at::Tensor x, long K, long S, long P,
                         bool include_pad);
at::Tensor avgpool2d_bwd(at::Tensor dy, long H, long W, long K, long S,
                         long P, bool include_pad);
at::Tensor global_avgpool_fwd(at::Tensor x);
at::Tensor global_avgpool_bwd(at::Tensor dy, long H, long W);
std::vector<at::Tensor> emb2_ln_fwd(at::Tensor ids, at::Tensor word,
                                    at::Tensor pos, at::Tensor w,
                                    at::Tensor b, double eps);
at::Tensor emb2_add_fwd(at::Tensor ids, at::Tensor word, at::Tensor pos);
std::vector<at::Tensor> emb2_bwd(at::Tensor dx, at::Tensor ids, long V,
                                 long P);
std::vector<at::Tensor> dropout_fwd(at::Tensor x, double p, int64_t seed,
                                    c10::optional<at::Tensor> seed_buf);
at::Tensor dropout_bwd(at::Tensor dy, at::Tensor mask, double p);
std::vector<at::Tensor> dropout_add_ln_fwd(at::Tensor z, at::Tensor a,
                                           at::Tensor w, at::Tensor bias,
                                           double eps, double p, int64_t seed,
                                           c10::optional<at::Tensor> seed_buf);
std::vector<at::Tensor> dropout_add_ln_bwd(at::Tensor dy, at::Tensor s,
                                           at::Tensor w, at::Tensor mean,
                                           at::Tensor rstd,
                                           at::Tensor maskbits, double p);
std::vector<at::Tensor> dropout_add_ln_bwd_dzsum(
    at::Tensor dy, at::Tensor s, at::Tensor w, at::Tensor mean,
    at::Tensor rstd, at::Tensor maskbits, double p, bool dzsum_bf16);
std::vector<at::Tensor> ce_fwd(at::Tensor logits, at::Tensor targets,
                               int64_t ignore_index);
at::Tensor ce_bwd(at::Tensor logits, at::Tensor targets, at::Tensor lse,
                  at::Tensor gscale, int64_t ignore_index);
std::vector<at::Tensor> mlm_head_fwd(at::Tensor h, at::Tensor W,
                                     at::Tensor b, at::Tensor targets,
                                     int64_t ignore_index);
std::vector<at::Tensor> mlm_head_bwd(at::Tensor dloss, at::Tensor logits_c,
                                     at::Tensor lse, at::Tensor hc,
                                     at::Tensor tc, at::Tensor pos,
                                     at::Tensor count, at::Tensor W);
std::tuple<at::Tensor, long, long> mt_build_table(
    std::vector<at::Tensor> ps, std::vector<at::Tensor> gs,
    std::vector<at::Tensor> ms, std::vector<at::Tensor> vs,
    std::vector<at::Tensor> masters);
std::tuple<at::Tensor, long, long> grad_build_table(
    std::vector<at::Tensor> gs);
void grad_sqnorm(at::Tensor table, long nchunks, long esize,
                 at::Tensor partials, long offset);
void grad_norm_finalize(at::Tensor partials, long n, at::Tensor stats,
                        double max_norm,
                        c10::optional<at::Tensor> max_norm_buf);
void scale_mt(at::Tensor table, long nchunks, long esize, at::Tensor gstats);
void fused_adam_graph(at::Tensor table, long nchunks, long esize,
                      at::Tensor lr_buf, double b1, double b2, double eps,
                      double wd, at::Tensor step_buf,
                      c10::optional<at::Tensor> gstats);
void fused_adam_table(at::Tensor table, long nchunks, long esize, double lr,
                      double b1, double b2, double eps, double wd, double bc1,
                      double bc2, c10::optional<at::Tensor> gstats);
void fused_sgd_table(at::Tensor table, long nchunks, long esize, double lr,
                     double momentum, double wd, bool nesterov,
                     c10::optional<at::Tensor> gstats);
void fused_lamb_table(at::Tensor table, long nchunks, long esize,
                      long ntensors, double lr, double b1, double b2,
                      double eps, double wd, double bc1, double bc2,
                      double clamp_trust, c10::optional<at::Tensor> gstats);
void fused_copy(std::vector<at::Tensor> srcs, std::vector<at::Tensor> dsts);
std::vector<at::Tensor> attn_fwd(at::Tensor q, at::Tensor k, at::Tensor v,
                                 at::Tensor mask, bool causal, double scale,
                                 c10::optional<at::Tensor> kv_len);
std::vector<at::Tensor> attn_bwd(at::Tensor q, at::Tensor k, at::Tensor v,
                                 at::Tensor o, at::Tensor dout,
                                 at::Tensor lse, at::Tensor mask, bool causal,
                                 double scale,
                                 c10::optional<at::Tensor> kv_len);
std::vector<at::Tensor> attn_fwd_qkv(at::Tensor qkv, at::Tensor mask,
                                     bool causal, double scale,
                                     double pdrop, int64_t dseed,
                                     c10::optional<at::Tensor> seed_buf,
                                     c10::optional<at::Tensor> kv_len);
at::Tensor attn_bwd_qkv(at::Tensor qkv, at::Tensor o, at::Tensor dout,
                        at::Tensor lse, at::Tensor mask, bool causal,
                        double scale, double pdrop,
                        c10::optional<at::Tensor> mbits,
                        c10::optional<at::Tensor> kv_len);
at::Tensor attn_mask_kv_len(at::Tensor mask);
at::Tensor mfma_probe(at::Tensor a, at::Tensor b);
at::Tensor tr16_probe();
at::Tensor mfma_mx_probe(at::Tensor a, at::Tensor b, int64_t sa, int64_t sb);

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("layernorm_fwd", &layernorm_fwd, "fused LayerNorm fwd (CDNA4)");
  m.def("layernorm_bwd", &layernorm_bwd, "fused LayerNorm bwd (CDNA4)");
  m.def("layernorm_add_fwd", &layernorm_add_fwd,
        "fused residual-add + LayerNorm fwd");
  m.def("layernorm_mx_fwd", &layernorm_mx_fwd,
        "fused LayerNorm fwd + MX fp8 quantisation of y: y, mean, rstd, q, "
        "s (bf16 x, hidden % 32 == 0)");
  m.def("bias_gelu_fwd", &bias_gelu_fwd, "fused bias+GELU fwd");
  m.def("bias_gelu_mx_fwd", &bias_gelu_mx_fwd,
        "fused bias+GELU fwd + MX fp8 quantisation of y: y, q, s (bf16 x, "
        "last dim % 32 == 0)");
  m.def("bias_gelu_bwd", &bias_gelu_bwd, "fused bias+GELU bwd");
  m.def("colsum_bf16", &colsum_bf16, "column sum bf16 -> fp32");
  m.def("bias_gelu_bwd_db", &bias_gelu_bwd_db,
        "fused bias+GELU bwd with in-pass bias-grad column reduction");
  m.def("batchnorm_fwd", &batchnorm_fwd, "fused BatchNorm2d fwd (NCHW)");
  m.def("batchnorm_bwd", &batchnorm_bwd, "fused BatchNorm2d bwd (NCHW)");
  m.def("batchnorm_relu_launch_constants", &batchnorm_relu_launch_constants,
        "(grid cap, block size, bytes per lane) of the BN+ReLU elementwise "
        "kernels");
  m.def("batchnorm_relu_fwd", &batchnorm_relu_fwd,
        "fused BatchNorm2d + [residual add] + ReLU fwd (NCHW)", py::arg("x"),
        py::arg("residual"), py::arg("w"), py::arg("b"),
        py::arg("running_mean"), py::arg("running_var"),
        py::arg("training"), py::arg("momentum"), py::arg("eps"));
  m.def("batchnorm_relu_bwd", &batchnorm_relu_bwd,
        "fused BatchNorm2d + [residual add] + ReLU bwd: dx, dw, db[, dr]");
  m.def("dropout_fwd", &dropout_fwd, "philox dropout fwd (replayable)",
        py::arg("x"), py::arg("p"), py::arg("seed"),
        py::arg("seed_buf") = py::none());
  m.def("dropout_bwd", &dropout_bwd, "dropout bwd");
  m.def("dropout_add_ln_fwd", &dropout_add_ln_fwd,
        "fused dropout + residual add + LayerNorm fwd (bf16, bit mask)",
        py::arg("z"), py::arg("a"), py::arg("w"), py::arg("bias"),
        py::arg("eps"), py::arg("p"), py::arg("seed"),
        py::arg("seed_buf") = py::none());
  m.def("dropout_add_ln_bwd", &dropout_add_ln_bwd,
        "fused dropout + residual add + LayerNorm bwd: dx, dz, dw, db");
  m.def("dropout_add_ln_bwd_dzsum", &dropout_add_ln_bwd_dzsum,
        "dropout_add_ln_bwd and dzsum = dz.sum(0), fp32 or bf16: dx, dz, dw, "
        "db, dzsum");
  m.def("conv2d_fwd", &conv2d_fwd,
        "implicit-GEMM MFMA conv fwd (bf16 NCHW)", py::arg("x"),
        py::arg("w"), py::arg("bias") = py::none(), py::arg("st") = 1,
        py::arg("pad") = 0, py::arg("relu") = false);
  m.def("conv2d_dgrad", &conv2d_dgrad, "implicit-GEMM MFMA conv dgrad");
  m.def("conv2d_wgrad", &conv2d_wgrad, "implicit-GEMM MFMA conv wgrad");
  m.def("gemm_nt_bf16", &gemm_nt_bf16,
        "bf16 MFMA GEMM x @ W^T (256^2 8-phase, fused bias/GELU epilogue)",
        py::arg("a"), py::arg("b"), py::arg("bias") = py::none(),
        py::arg("epi") = 0);
  m.def("gemm_wgrad_bf16", &gemm_wgrad_bf16,
        "split-K wgrad dW = dy^T @ x (tr16 transpose reads, fp32 atomics)");
  m.def("gemm_nt_bf16_rows", &gemm_nt_bf16_rows,
        "gemm_nt_bf16 into the caller's C (row stride C.size(1)), rows "
        "below a device-side int32 limit only; epi 0 or 1",
        py::arg("a"), py::arg("b"), py::arg("bias"), py::arg("epi"),
        py::arg("c"), py::arg("row_limit"));
  m.def("gemm_wgrad_bf16_rows", &gemm_wgrad_bf16_rows,
        "gemm_wgrad_bf16 over rows [0, round_up(min(*row_bound, M), 64))",
        py::arg("dy"), py::arg("x"), py::arg("row_bound"));
  m.def("mx_quant", &mx_quant,
        "bf16 -> MX fp8 (e4m3 + per-32 e8m0 scales)");
  // bias: optional bf16 or fp32 (N,), added in the epilogue as
  // bf16(float(bf16(acc)) + bias): bit-identical to a separate bf16 add
  m.def("mx_gemm", &mx_gemm, "MX fp8 GEMM: x @ W^T, 32x32x64 scaled MFMA",
        py::arg("x"), py::arg("xs"), py::arg("w"), py::arg("ws"),
        py::arg("bias") = py::none());
  m.def("mx_gemm2", &mx_gemm2,
        "LDS-staged MX fp8 GEMM (256^2 4-phase, scaled 32x32x64 MFMA)",
        py::arg("xq"), py::arg("xs"), py::arg("wq"), py::arg("ws"),
        py::arg("bias") = py::none());
  m.def("mx_scale_probe", &mx_scale_probe,
        "per-lane scale-byte semantics probe");
  m.def("softmax_fwd", &softmax_fwd, "standalone softmax fwd (last dim)");
  m.def("softmax_bwd", &softmax_bwd, "standalone softmax bwd");
  m.def("maxpool2d_fwd", &maxpool2d_fwd, "MaxPool2d fwd (+argmax idx)");
  m.def("maxpool2d_bwd", &maxpool2d_bwd, "MaxPool2d bwd (gather)");
  m.def("avgpool2d_fwd", &avgpool2d_fwd, "AvgPool2d fwd");
  m.def("avgpool2d_bwd", &avgpool2d_bwd, "AvgPool2d bwd");
  m.def("global_avgpool_fwd", &global_avgpool_fwd,
        "global (adaptive 1x1) avg pool fwd");
  m.def("global_avgpool_bwd", &global_avgpool_bwd, "global avg pool bwd");
  m.def("emb2_ln_fwd", &emb2_ln_fwd,
        "fused word+pos embedding gather + LayerNorm fwd");
  m.def("emb2_add_fwd", &emb2_add_fwd, "fused word+pos embedding gather");
  m.def("emb2_bwd", &emb2_bwd,
        "embedding bwd: dword scatter-add + dpos batch reduction");
  m.def("ce_fwd", &ce_fwd, "fused softmax cross-entropy fwd");
  m.def("ce_bwd", &ce_bwd, "fused softmax cross-entropy bwd");
  m.def("mlm_head_fwd", &mlm_head_fwd,
        "sparse MLM head fwd: decoder GEMM + CE on the non-ignored rows "
        "(device-side live count, graph-capturable)");
  m.def("mlm_head_bwd", &mlm_head_bwd,
        "sparse MLM head bwd: dh, dW, db (consumes the saved logits)");
  m.def("fused_adam_graph", &fused_adam_graph,
        "multi-tensor Adam with device lr/step buffers (hipGraph mode)",
        py::arg("table"), py::arg("nchunks"), py::arg("esize"),
        py::arg("lr_buf"), py::arg("b1"), py::arg("b2"), py::arg("eps"),
        py::arg("wd"), py::arg("step_buf"), py::arg("gstats") = py::none());
  m.def("mt_build_table", &mt_build_table,
        "prebuild the device chunk table (any fused optimizer)");
  m.def("grad_build_table", &grad_build_table,
        "grads-only device chunk table (clip_grad_norm_)");
  m.def("grad_sqnorm", &grad_sqnorm,
        "multi-tensor per-chunk sum of squared grads -> partials");
  m.def("grad_norm_finalize", &grad_norm_finalize,
        "partials -> [norm, clip coefficient, non-finite count]",
        py::arg("partials"), py::arg("n"), py::arg("stats"),
        py::arg("max_norm"), py::arg("max_norm_buf") = py::none());
  m.def("scale_mt", &scale_mt, "multi-tensor in-place g *= stats[1]");
  m.def("fused_adam_table", &fused_adam_table,
        "multi-tensor Adam from a prebuilt table (+ clip coefficient)",
        py::arg("table"), py::arg("nchunks"), py::arg("esize"),
        py::arg("lr"), py::arg("b1"), py::arg("b2"), py::arg("eps"),
        py::arg("wd"), py::arg("bc1"), py::arg("bc2"),
        py::arg("gstats") = py::none());
  m.def("fused_sgd_table", &fused_sgd_table,
        "multi-tensor SGD from a prebuilt table (+ clip coefficient)",
        py::arg("table"), py::arg("nchunks"), py::arg("esize"),
        py::arg("lr"), py::arg("momentum"), py::arg("wd"),
        py::arg("nesterov"), py::arg("gstats") = py::none());
  m.def("fused_lamb_table", &fused_lamb_table,
        "multi-tensor LAMB from a prebuilt table (+ clip coefficient)",
        py::arg("table"), py::arg("nchunks"), py::arg("esize"),
        py::arg("ntensors"), py::arg("lr"), py::arg("b1"), py::arg("b2"),
        py::arg("eps"), py::arg("wd"), py::arg("bc1"), py::arg("bc2"),
        py::arg("clamp_trust"), py::arg("gstats") = py::none());
  m.def("fused_copy", &fused_copy, "multi-tensor device copy");
  // kv_len: optional int32[B] per-sequence key counts; keys past it are
  // skipped (whole tiles) or scored -inf (ragged tile)
  m.def("attn_fwd", &attn_fwd,
        py::arg("q"), py::arg("k"), py::arg("v"), py::arg("mask"),
        py::arg("causal"), py::arg("scale"), py::arg("kv_len") = py::none(),
        "flash attention fwd (bf16, MFMA)");
  m.def("attn_bwd", &attn_bwd,
        py::arg("q"), py::arg("k"), py::arg("v"), py::arg("o"),
        py::arg("dout"), py::arg("lse"), py::arg("mask"), py::arg("causal"),
        py::arg("scale"), py::arg("kv_len") = py::none(),
        "flash attention bwd (bf16, MFMA, D=64)");
  m.def("attn_fwd_qkv", &attn_fwd_qkv,
        py::arg("qkv"), py::arg("mask"), py::arg("causal"),
        py::arg("scale"), py::arg("pdrop") = 0.0, py::arg("dseed") = 0,
        py::arg("seed_buf") = py::none(), py::arg("kv_len") = py::none(),
        "flash attention fwd, packed (B,S,3,H,D) qkv -> (B,S,H,D)");
  m.def("attn_bwd_qkv", &attn_bwd_qkv,
        py::arg("qkv"), py::arg("o"), py::arg("dout"), py::arg("lse"),
        py::arg("mask"), py::arg("causal"), py::arg("scale"),
        py::arg("pdrop") = 0.0, py::arg("mbits") = py::none(),
        py::arg("kv_len") = py::none(),
        "flash attention bwd, packed qkv -> dqkv");
  m.def("attn_mask_kv_len", &attn_mask_kv_len, py::arg("mask"),
        "additive (B,S) padding mask -> int32[B] key horizon");
  m.def("mfma_probe", &mfma_probe, "32x32x16 bf16 MFMA layout probe");
  m.def("tr16_probe", &tr16_probe, "ds_read_b64_tr_b16 mapping probe");
  m.def("mfma_mx_probe", &mfma_mx_probe,
        "32x32x64 MX-scaled fp8 MFMA layout probe");
}
