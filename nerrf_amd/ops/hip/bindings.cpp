// Torch extension bindings for the nerrf-amd CDNA4 kernels.
#include <torch/extension.h>

#include <limits>

#include <ATen/hip/HIPContext.h>
#include <hip/hip_runtime.h>

#include "mcts_params.h"

namespace nerrf {
void launch_mcts(const float*, const float*, const float*, float, float,
                 const PlannerParamsDev&, int, int, int*, float*, int*, float*,
                 hipStream_t);
void launch_eval_plans(const float*, const float*, const float*, float, float,
                       const PlannerParamsDev&, const int*, int, int, float*,
                       hipStream_t);
void launch_plan_oracle(const float*, const float*, const float*, const float*,
                        const float*, const PlannerParamsDev&, int, int, int,
                        float*, int*, unsigned*, hipStream_t);
void launch_gather_mean_fwd(const void*, const long*, const float*, void*, int,
                            int, int, bool, hipStream_t);
void launch_gather_mean_bwd(const void*, const long*, const float*, float*,
                            int, int, int, bool, hipStream_t);
void launch_gather_mean_bwd_csr(const void*, const long*, const long*,
                                const float*, float*, long, int, bool,
                                hipStream_t);
void launch_lstm_pointwise_fwd(const void*, const void*, const void*,
                               const void*, const void*, const float*, void*,
                               void*, void*, long, int, long, long, long,
                               long, bool, hipStream_t);
bool launch_lstm_pointwise_bwd(const void*, const void*, const void*,
                               const void*, const void*, const float*, void*,
                               void*, void*, float*, long, long, int, long,
                               long, long, long, bool, hipStream_t);
void launch_lstm_step_fused(const void*, const void*, const void*, const void*,
                            const void*, const float*, void*, void*, void*,
                            int, bool, hipStream_t);
void launch_lstm_rec_fwd(const void*, const void*, const void*, const void*,
                         const void*, const float*, void*, void*, void*, int,
                         long, long, long, hipStream_t);
void launch_lstm_rec_bwd(const void*, const void*, const void*, const void*,
                         const void*, const void*, const float*, void*, void*,
                         void*, int, long, long, hipStream_t);
void launch_rec_gemm_fwd(const void*, const void*, void*, long, long, long,
                         hipStream_t);
void launch_rec_gemm_dgrad(const void*, const void*, const void*, void*,
                           long, long, hipStream_t);
void launch_proj_fwd_dual(const void*, const void*, const void*, void*, void*,
                          long, long, hipStream_t);
void launch_proj_dgrad_dual(const void*, const void*, const void*, const void*,
                            void*, long, hipStream_t);
void launch_proj_wgrad(const void*, const void*, const void*, float*, float*,
                       long, long, int, hipStream_t);
void launch_event_scatter(const long*, const long*, const signed char*,
                          const float*, const int*, float*, int*, int*, long,
                          hipStream_t);
void launch_feature_assemble(const float*, const int*, const int*,
                             const float*, const float*, const float*,
                             const unsigned char*, const signed char*, float*,
                             float, int, hipStream_t);
void launch_sage_layer_fwd(const void*, const long*, const float*, const void*,
                           const void*, const void*, const void*, const void*,
                           void*, int, int, hipStream_t);
void launch_edge_head_fwd(const void*, const long*, const long*, const float*,
                          const float*, const void*, const float*, const void*,
                          const void*, const void*, float*, long, hipStream_t);
void launch_edge_attr(const float*, const long*, const long*,
                      unsigned long long*, int*, long*, float*, long, long,
                      long, bool, float, hipStream_t);
void launch_sage_ln_act_fwd(const void*, const void*, const void*, const void*,
                            const void*, void*, void*, float*, unsigned char*,
                            long, float, unsigned, hipStream_t);
void launch_sage_ln_act_bwd(const void*, const void*, const float*,
                            const void*, void*, float*, float*, long, float,
                            unsigned, hipStream_t);
}  // namespace nerrf

namespace {

bool is_bf16(const torch::Tensor& t) {
  TORCH_CHECK(
      t.scalar_type() == torch::kBFloat16 || t.scalar_type() == torch::kFloat32,
      "nerrf kernels support bf16/fp32, got ", t.scalar_type());
  return t.scalar_type() == torch::kBFloat16;
}

void check_gpu_contig(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be on GPU");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
}

// 2D tensor whose rows may be strided (last dim contiguous) — the dual-
// direction LSTM reads gate slabs / writes hidden halves inside wider
// concatenated buffers.
long row_stride_checked(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be on GPU");
  TORCH_CHECK(t.dim() == 2 && t.stride(1) == 1, name,
              " must be 2D with contiguous rows");
  return t.stride(0);
}

torch::Tensor gather_mean_fwd(torch::Tensor h, torch::Tensor idx,
                              torch::Tensor w) {
  check_gpu_contig(h, "h");
  check_gpu_contig(idx, "idx");
  check_gpu_contig(w, "w");
  TORCH_CHECK(idx.scalar_type() == torch::kInt64, "idx must be int64");
  const int n = idx.size(0);
  const int k = idx.size(1);
  const int dim = h.size(1);
  TORCH_CHECK(k <= 64, "fanout K must be <= 64 (wave-resident), got ", k);
  TORCH_CHECK(dim <= 512, "feature dim must be <= 512, got ", dim);
  auto wf = w.scalar_type() == torch::kFloat32 ? w : w.to(torch::kFloat32);
  auto out = torch::empty({n, dim}, h.options());
  auto stream = at::hip::getCurrentHIPStream();
  nerrf::launch_gather_mean_fwd(h.data_ptr(), idx.data_ptr<long>(),
                                wf.data_ptr<float>(), out.data_ptr(), n, dim,
                                k, is_bf16(h), stream.stream());
  return out;
}

torch::Tensor gather_mean_bwd(torch::Tensor grad_out, torch::Tensor idx,
                              torch::Tensor w, long num_nodes) {
  check_gpu_contig(grad_out, "grad_out");
  check_gpu_contig(idx, "idx");
  const int n = idx.size(0);
  const int k = idx.size(1);
  const int dim = grad_out.size(1);
  auto wf = w.scalar_type() == torch::kFloat32 ? w.contiguous()
                                               : w.to(torch::kFloat32).contiguous();
  auto ws = torch::zeros({num_nodes, dim},
                         grad_out.options().dtype(torch::kFloat32));
  auto stream = at::hip::getCurrentHIPStream();
  nerrf::launch_gather_mean_bwd(grad_out.data_ptr(), idx.data_ptr<long>(),
                                wf.data_ptr<float>(), ws.data_ptr<float>(), n,
                                dim, k, is_bf16(grad_out), stream.stream());
  return ws.to(grad_out.scalar_type());
}

torch::Tensor gather_mean_bwd_csr(torch::Tensor grad_out,
                                  torch::Tensor rev_dst,
                                  torch::Tensor rev_src, torch::Tensor rev_w,
                                  long num_nodes) {
  check_gpu_contig(grad_out, "grad_out");
  check_gpu_contig(rev_dst, "rev_dst");
  check_gpu_contig(rev_src, "rev_src");
  check_gpu_contig(rev_w, "rev_w");
  const int dim = grad_out.size(1);
  const long n_entries = rev_dst.numel();
  auto ws = torch::zeros({num_nodes, (long)dim},
                         grad_out.options().dtype(torch::kFloat32));
  auto stream = at::hip::getCurrentHIPStream();
  nerrf::launch_gather_mean_bwd_csr(
      grad_out.data_ptr(), rev_dst.data_ptr<long>(), rev_src.data_ptr<long>(),
      rev_w.data_ptr<float>(), ws.data_ptr<float>(), n_entries, dim,
      is_bf16(grad_out), stream.stream());
  return ws.to(grad_out.scalar_type());
}

// The vectorised pointwise kernels move 16 bytes per access.  Row strides
// that are multiples of the vector width are not enough: a tensor that is a
// row slice of a packed buffer starts at a row offset, so its base address
// is checked too.
void check_vec_base(const torch::Tensor& t, bool vec, const char* name) {
  TORCH_CHECK(!vec || t.numel() == 0 ||
                  reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0,
              name, " must start on a 16-byte boundary");
}

// Writes into caller-provided (h_out, c_out, gates_act) so the sequence loop
// can target time-major buffers directly (no per-step allocation or copy).
// The step covers h_out.size(0) rows.  prev_rows (< 0: all rows) is how many
// of them have a previous state: hg, c_prev and h_prev need only that many
// rows, and rows beyond start from zero without reading any of the three.
void lstm_pointwise_fwd(torch::Tensor hg, torch::Tensor xg, torch::Tensor bias,
                        torch::Tensor c_prev, torch::Tensor h_prev,
                        torch::Tensor mask, torch::Tensor h_out,
                        torch::Tensor c_out, torch::Tensor gates_act,
                        long prev_rows) {
  check_gpu_contig(hg, "hg");
  const long xg_stride = row_stride_checked(xg, "xg");
  check_gpu_contig(c_prev, "c_prev");
  const long hprev_stride = row_stride_checked(h_prev, "h_prev");
  const long hout_stride = row_stride_checked(h_out, "h_out");
  check_gpu_contig(c_out, "c_out");
  const bool want_gates = gates_act.numel() > 0;
  if (want_gates) check_gpu_contig(gates_act, "gates_act");
  const long batch = c_out.size(0);
  const int hdim = c_out.size(1);
  if (prev_rows < 0) prev_rows = batch;
  TORCH_CHECK(prev_rows <= batch, "prev_rows exceeds the step's rows");
  TORCH_CHECK(hg.dim() == 2 && c_prev.dim() == 2 && hg.size(0) >= prev_rows &&
                  c_prev.size(0) >= prev_rows && h_prev.size(0) >= prev_rows &&
                  c_prev.size(1) == hdim && h_prev.size(1) == hdim,
              "hg/c_prev/h_prev must cover prev_rows rows");
  TORCH_CHECK(hg.size(1) == 4 * hdim && xg.size(1) == 4 * hdim,
              "hg/xg must be [B, 4H]");
  TORCH_CHECK(xg.size(0) == batch && h_out.size(0) == batch &&
                  h_out.size(1) == hdim &&
                  (!want_gates || gates_act.size(0) == batch),
              "xg/h_out/c_out/gates_act must have the step's rows");
  TORCH_CHECK(bias.numel() == 4 * hdim, "bias must be [4H]");
  const float* mask_ptr = nullptr;
  torch::Tensor mf;
  if (mask.numel() > 0) {
    mf = mask.scalar_type() == torch::kFloat32 ? mask.contiguous()
                                               : mask.to(torch::kFloat32).contiguous();
    TORCH_CHECK(mf.numel() == batch, "mask must be [B]");
    mask_ptr = mf.data_ptr<float>();
  }
  auto bc = bias.contiguous();
  const bool bf16 = is_bf16(hg);
  const int v = bf16 ? 8 : 4;
  const bool vec = hdim % v == 0 && xg_stride % v == 0 &&
                   hout_stride % v == 0 && hprev_stride % v == 0;
  check_vec_base(hg, vec, "hg");
  check_vec_base(xg, vec, "xg");
  check_vec_base(bc, vec, "bias");
  check_vec_base(c_prev, vec, "c_prev");
  check_vec_base(h_prev, vec, "h_prev");
  check_vec_base(h_out, vec, "h_out");
  check_vec_base(c_out, vec, "c_out");
  check_vec_base(gates_act, vec, "gates_act");
  auto stream = at::hip::getCurrentHIPStream();
  nerrf::launch_lstm_pointwise_fwd(
      hg.data_ptr(), xg.data_ptr(), bc.data_ptr(), c_prev.data_ptr(),
      h_prev.data_ptr(), mask_ptr, h_out.data_ptr(), c_out.data_ptr(),
      want_gates ? gates_act.data_ptr() : nullptr, batch, hdim, xg_stride,
      hout_stride, hprev_stride, prev_rows, bf16, stream.stream());
}

// grad_out_t (may be empty): this timestep's dL/dh, folded in-kernel so the
// sequence backward needs no separate elementwise add per step.
// bias_accum (optional, may be empty): contiguous f32 slab [P, 4H], P >= 1.
// The kernel runs on min(P, blocks needed) blocks and block p ADDS its
// sum over rows of the stored grad_gates into slab row p (plain stores, no
// atomics; rows beyond the grid are not touched), so one slab accumulates
// over the timesteps of a sequence and the caller's bias gradient is
// slab.sum(0) — no whole-tensor gg.sum(0) re-read.  Returns true when the
// fused accumulation ran: it needs the vectorised path and
// 256 % (H/V) == 0 (V = 8 for bf16, 4 for f32); otherwise the slab is left
// untouched and false is returned.
// The step covers gates_act.size(0) rows.  in_rows (< 0: all rows): rows
// with an incoming recurrent gradient — grad_h and grad_c need only that
// many rows and the rest take 0 without a read.  prev_rows (< 0: all rows):
// rows whose previous cell state exists; c_prev needs only that many.
// grad_h_pass may be empty when there is no mask (it is identically zero
// then): the store is skipped.
bool lstm_pointwise_bwd(torch::Tensor grad_h, torch::Tensor grad_out_t,
                        torch::Tensor grad_c, torch::Tensor gates_act,
                        torch::Tensor c_prev, torch::Tensor mask,
                        torch::Tensor grad_gates, torch::Tensor grad_c_prev,
                        torch::Tensor grad_h_pass, torch::Tensor bias_accum,
                        long in_rows, long prev_rows) {
  check_gpu_contig(grad_h, "grad_h");
  check_gpu_contig(grad_c, "grad_c");
  check_gpu_contig(gates_act, "gates_act");
  check_gpu_contig(c_prev, "c_prev");
  const long gg_stride = row_stride_checked(grad_gates, "grad_gates");
  check_gpu_contig(grad_c_prev, "grad_c_prev");
  const bool want_pass = grad_h_pass.numel() > 0;
  if (want_pass) check_gpu_contig(grad_h_pass, "grad_h_pass");
  TORCH_CHECK(gates_act.dim() == 2 && gates_act.size(1) % 4 == 0,
              "gates_act must be [B, 4H]");
  const long batch = gates_act.size(0);
  const int hdim = gates_act.size(1) / 4;
  if (in_rows < 0) in_rows = batch;
  if (prev_rows < 0) prev_rows = batch;
  TORCH_CHECK(in_rows <= batch && prev_rows <= batch,
              "in_rows/prev_rows exceed the step's rows");
  TORCH_CHECK(grad_h.numel() >= in_rows * hdim && grad_c.numel() >= in_rows * hdim,
              "grad_h/grad_c must cover in_rows rows");
  TORCH_CHECK(c_prev.numel() >= prev_rows * hdim,
              "c_prev must cover prev_rows rows");
  TORCH_CHECK(grad_gates.size(0) == batch && grad_gates.size(1) == 4 * hdim &&
                  grad_c_prev.numel() >= batch * hdim &&
                  (!want_pass || grad_h_pass.numel() >= batch * hdim),
              "grad_gates/grad_c_prev/grad_h_pass must have the step's rows");
  TORCH_CHECK(want_pass || mask.numel() == 0,
              "grad_h_pass is required with a mask");
  const float* mask_ptr = nullptr;
  torch::Tensor mf;
  if (mask.numel() > 0) {
    mf = mask.scalar_type() == torch::kFloat32 ? mask.contiguous()
                                               : mask.to(torch::kFloat32).contiguous();
    TORCH_CHECK(mf.numel() == batch, "mask must be [B]");
    mask_ptr = mf.data_ptr<float>();
  }
  auto stream = at::hip::getCurrentHIPStream();
  const void* got = grad_out_t.numel() ? grad_out_t.data_ptr() : nullptr;
  long gout_stride = hdim;
  if (grad_out_t.numel()) {
    gout_stride = row_stride_checked(grad_out_t, "grad_out_t");
    TORCH_CHECK(grad_out_t.size(0) == batch && grad_out_t.size(1) == hdim,
                "grad_out_t must be [B, H]");
  }
  float* bias_ptr = nullptr;
  long accum_rows = 0;
  if (bias_accum.numel() > 0) {
    check_gpu_contig(bias_accum, "bias_accum");
    TORCH_CHECK(bias_accum.scalar_type() == torch::kFloat32 && hdim > 0 &&
                    bias_accum.numel() % (4 * (long)hdim) == 0,
                "bias_accum must be a contiguous f32 slab [P, 4H]");
    bias_ptr = bias_accum.data_ptr<float>();
    accum_rows = bias_accum.numel() / (4 * (long)hdim);
  }
  const bool bf16 = is_bf16(grad_h);
  const int v = bf16 ? 8 : 4;
  const bool vec = hdim % v == 0 && gout_stride % v == 0 && gg_stride % v == 0;
  check_vec_base(grad_h, vec, "grad_h");
  check_vec_base(grad_out_t, vec, "grad_out_t");
  check_vec_base(grad_c, vec, "grad_c");
  check_vec_base(gates_act, vec, "gates_act");
  check_vec_base(c_prev, vec, "c_prev");
  check_vec_base(grad_gates, vec, "grad_gates");
  check_vec_base(grad_c_prev, vec, "grad_c_prev");
  check_vec_base(grad_h_pass, vec, "grad_h_pass");
  return nerrf::launch_lstm_pointwise_bwd(
      grad_h.data_ptr(), got, grad_c.data_ptr(), gates_act.data_ptr(),
      c_prev.data_ptr(), mask_ptr, grad_gates.data_ptr(),
      grad_c_prev.data_ptr(), want_pass ? grad_h_pass.data_ptr() : nullptr,
      bias_ptr, accum_rows, batch, hdim, gout_stride, gg_stride, in_rows,
      prev_rows, bf16, stream.stream());
}

// Fused recurrent step (bf16, H == 256): h_prev @ W_hh^T + LSTM pointwise
// in one launch — the [B, 4H] pre-activation slab never touches HBM.
void lstm_rec_fwd(torch::Tensor h_prev, torch::Tensor w_hh, torch::Tensor xg,
                  torch::Tensor bias, torch::Tensor c_prev, torch::Tensor mask,
                  torch::Tensor h_out, torch::Tensor c_out,
                  torch::Tensor gates_act) {
  const long hprev_stride = row_stride_checked(h_prev, "h_prev");
  const long xg_stride = row_stride_checked(xg, "xg");
  const long hout_stride = row_stride_checked(h_out, "h_out");
  check_gpu_contig(w_hh, "w_hh");
  check_gpu_contig(c_prev, "c_prev");
  check_gpu_contig(c_out, "c_out");
  const bool want_gates = gates_act.numel() > 0;
  if (want_gates) check_gpu_contig(gates_act, "gates_act");
  for (auto* t : {&h_prev, &w_hh, &xg, &c_prev, &h_out, &c_out}) {
    TORCH_CHECK(t->scalar_type() == torch::kBFloat16,
                "lstm_rec_fwd is bf16-only");
  }
  const long batch = c_prev.size(0);
  TORCH_CHECK(c_prev.size(1) == 256 && h_prev.size(1) == 256 &&
                  xg.size(1) == 1024 && w_hh.size(0) == 1024 &&
                  w_hh.size(1) == 256,
              "lstm_rec_fwd requires H=256");
  const float* mask_ptr = nullptr;
  torch::Tensor mf;
  if (mask.numel() > 0) {
    mf = mask.scalar_type() == torch::kFloat32 ? mask.contiguous()
                                               : mask.to(torch::kFloat32).contiguous();
    mask_ptr = mf.data_ptr<float>();
  }
  auto bc = bias.contiguous();
  auto stream = at::hip::getCurrentHIPStream();
  nerrf::launch_lstm_rec_fwd(
      h_prev.data_ptr(), w_hh.data_ptr(), xg.data_ptr(), bc.data_ptr(),
      c_prev.data_ptr(), mask_ptr, h_out.data_ptr(), c_out.data_ptr(),
      want_gates ? gates_act.data_ptr() : nullptr, (int)batch, hprev_stride,
      xg_stride, hout_stride, stream.stream());
}

// Fused recurrent backward (bf16, H == 256): gate grads + grad_c_prev +
// grad_h = ghp + grad_gates @ W_hh in one launch.
void lstm_rec_bwd(torch::Tensor grad_h, torch::Tensor grad_out_t,
                  torch::Tensor grad_c, torch::Tensor gates_act,
                  torch::Tensor c_prev, torch::Tensor w_hh_t,
                  torch::Tensor mask, torch::Tensor grad_gates,
                  torch::Tensor grad_c_prev, torch::Tensor grad_h_out) {
  check_gpu_contig(grad_h, "grad_h");
  check_gpu_contig(grad_c, "grad_c");
  check_gpu_contig(gates_act, "gates_act");
  check_gpu_contig(c_prev, "c_prev");
  check_gpu_contig(w_hh_t, "w_hh_t");
  const long gg_stride = row_stride_checked(grad_gates, "grad_gates");
  check_gpu_contig(grad_c_prev, "grad_c_prev");
  check_gpu_contig(grad_h_out, "grad_h_out");
  for (auto* t : {&grad_h, &grad_c, &gates_act, &c_prev, &w_hh_t}) {
    TORCH_CHECK(t->scalar_type() == torch::kBFloat16,
                "lstm_rec_bwd is bf16-only");
  }
  const long batch = c_prev.size(0);
  TORCH_CHECK(c_prev.size(1) == 256 && gates_act.size(1) == 1024 &&
                  w_hh_t.size(0) == 256 && w_hh_t.size(1) == 1024,
              "lstm_rec_bwd requires H=256 and w_hh_t = W_hh^T contiguous");
  const float* mask_ptr = nullptr;
  torch::Tensor mf;
  if (mask.numel() > 0) {
    mf = mask.scalar_type() == torch::kFloat32 ? mask.contiguous()
                                               : mask.to(torch::kFloat32).contiguous();
    mask_ptr = mf.data_ptr<float>();
  }
  auto stream = at::hip::getCurrentHIPStream();
  const void* got = grad_out_t.numel() ? grad_out_t.data_ptr() : nullptr;
  long gout_stride = 256;
  if (grad_out_t.numel()) gout_stride = row_stride_checked(grad_out_t, "grad_out_t");
  nerrf::launch_lstm_rec_bwd(
      grad_h.data_ptr(), got, grad_c.data_ptr(), gates_act.data_ptr(),
      c_prev.data_ptr(), w_hh_t.data_ptr(), mask_ptr, grad_gates.data_ptr(),
      grad_c_prev.data_ptr(), grad_h_out.data_ptr(), (int)batch, gout_stride,
      gg_stride, stream.stream());
}

// Fully-fused MFMA step (bf16, H == 256). Writes into caller buffers.
void lstm_step_fused(torch::Tensor h_prev, torch::Tensor w_hh, torch::Tensor xg,
                     torch::Tensor bias, torch::Tensor c_prev,
                     torch::Tensor mask, torch::Tensor h_out,
                     torch::Tensor c_out, torch::Tensor gates_act, bool raw) {
  for (auto* t : {&h_prev, &w_hh, &xg, &c_prev, &h_out, &c_out, &gates_act}) {
    check_gpu_contig(*t, "lstm_step_fused arg");
    TORCH_CHECK(t->scalar_type() == torch::kBFloat16,
                "lstm_step_fused is bf16-only");
  }
  const int batch = h_prev.size(0);
  TORCH_CHECK(h_prev.size(1) == 256 && xg.size(1) == 1024,
              "lstm_step_fused requires H=256 (got h ", h_prev.size(1), ")");
  TORCH_CHECK(w_hh.dim() == 3 && w_hh.size(0) == 8 && w_hh.size(1) == 1024 &&
                  w_hh.size(2) == 32,
              "w must be k-tiled [8,1024,32] (w_hh.reshape(1024,8,32)"
              ".permute(1,0,2).contiguous())");
  const float* mask_ptr = nullptr;
  torch::Tensor mf;
  if (mask.numel() > 0) {
    mf = mask.scalar_type() == torch::kFloat32 ? mask.contiguous()
                                               : mask.to(torch::kFloat32).contiguous();
    mask_ptr = mf.data_ptr<float>();
  }
  auto bc = bias.contiguous();
  auto stream = at::hip::getCurrentHIPStream();
  nerrf::launch_lstm_step_fused(
      h_prev.data_ptr(), w_hh.data_ptr(), xg.data_ptr(), bc.data_ptr(),
      c_prev.data_ptr(), mask_ptr, h_out.data_ptr(), c_out.data_ptr(),
      gates_act.data_ptr(), batch, raw, stream.stream());
}

// Recurrent-step GEMM: c = a @ w^T with [M,256] x [1024,256] (bf16; A and C
// may be row-strided column slabs of wider buffers).
void rec_gemm_fwd(torch::Tensor a, torch::Tensor w, torch::Tensor c) {
  const long a_stride = row_stride_checked(a, "a");
  const long c_stride = row_stride_checked(c, "c");
  check_gpu_contig(w, "w");
  TORCH_CHECK(a.scalar_type() == torch::kBFloat16, "rec_gemm_fwd is bf16-only");
  TORCH_CHECK(a.size(1) == 256 && w.size(0) == 1024 && w.size(1) == 256 &&
                  c.size(1) == 1024 && c.size(0) == a.size(0),
              "rec_gemm_fwd requires [M,256] x [1024,256] -> [M,1024]");
  TORCH_CHECK(a_stride % 8 == 0 && c_stride % 8 == 0,
              "rec_gemm_fwd needs 16-B aligned rows");
  check_vec_base(a, true, "a");
  check_vec_base(c, true, "c");
  auto stream = at::hip::getCurrentHIPStream();
  nerrf::launch_rec_gemm_fwd(a.data_ptr(), w.data_ptr(), c.data_ptr(),
                             a.size(0), a_stride, c_stride, stream.stream());
}

// Recurrence backward dgrad: c = a @ wt^T + d with [M,1024] x [256,1024]
// (wt = W_hh^T contiguous; d optional addend, pass an empty tensor to skip).
void rec_gemm_dgrad(torch::Tensor a, torch::Tensor wt, torch::Tensor d,
                    torch::Tensor c) {
  const long a_stride = row_stride_checked(a, "a");
  check_gpu_contig(wt, "wt");
  check_gpu_contig(c, "c");
  TORCH_CHECK(a.scalar_type() == torch::kBFloat16, "rec_gemm_dgrad is bf16-only");
  TORCH_CHECK(a.size(1) == 1024 && wt.size(0) == 256 && wt.size(1) == 1024 &&
                  c.size(1) == 256 && c.size(0) == a.size(0),
              "rec_gemm_dgrad requires [M,1024] x [256,1024] -> [M,256]");
  TORCH_CHECK(a_stride % 8 == 0, "rec_gemm_dgrad needs 16-B aligned rows");
  const bool has_d = d.numel() > 0;
  if (has_d) {
    check_gpu_contig(d, "d");
    TORCH_CHECK(d.sizes() == c.sizes(), "addend shape must match output");
  }
  auto stream = at::hip::getCurrentHIPStream();
  nerrf::launch_rec_gemm_dgrad(a.data_ptr(), wt.data_ptr(),
                               has_d ? d.data_ptr() : nullptr, c.data_ptr(),
                               a.size(0), a_stride, stream.stream());
}

// Dual-direction LSTM input projection: c1 = a @ w1^T, c2 = a @ w2^T in one
// launch (A staged in LDS once; K=512, N=1024 per direction, bf16).
void proj_fwd_dual(torch::Tensor a, torch::Tensor w1, torch::Tensor w2,
                   torch::Tensor c1, torch::Tensor c2) {
  const long a_stride = row_stride_checked(a, "a");
  check_gpu_contig(w1, "w1");
  check_gpu_contig(c1, "c1");
  TORCH_CHECK(a.scalar_type() == torch::kBFloat16, "proj_fwd_dual is bf16-only");
  TORCH_CHECK(a.size(1) == 512 && w1.size(0) == 1024 && w1.size(1) == 512 &&
                  c1.size(1) == 1024,
              "proj_fwd_dual requires [M,512] x [1024,512]");
  const bool dual = w2.numel() > 0;
  if (dual) {
    check_gpu_contig(w2, "w2");
    check_gpu_contig(c2, "c2");
    TORCH_CHECK(w2.sizes() == w1.sizes() && c2.sizes() == c1.sizes(),
                "dual shapes must match");
  }
  auto stream = at::hip::getCurrentHIPStream();
  nerrf::launch_proj_fwd_dual(
      a.data_ptr(), w1.data_ptr(), dual ? w2.data_ptr() : nullptr,
      c1.data_ptr(), dual ? c2.data_ptr() : nullptr, a.size(0), a_stride,
      stream.stream());
}

// Dual-direction input-projection dgrad: c = a1 @ w1t^T + a2 @ w2t^T
// (w*t = W^T contiguous [512, 1024]).
void proj_dgrad_dual(torch::Tensor a1, torch::Tensor a2, torch::Tensor w1t,
                     torch::Tensor w2t, torch::Tensor c) {
  check_gpu_contig(a1, "a1");
  check_gpu_contig(w1t, "w1t");
  check_gpu_contig(c, "c");
  TORCH_CHECK(a1.scalar_type() == torch::kBFloat16, "proj_dgrad_dual is bf16-only");
  TORCH_CHECK(a1.size(1) == 1024 && w1t.size(0) == 512 && w1t.size(1) == 1024 &&
                  c.size(1) == 512,
              "proj_dgrad_dual requires [M,1024] x [512,1024]");
  const bool dual = a2.numel() > 0;
  if (dual) {
    check_gpu_contig(a2, "a2");
    check_gpu_contig(w2t, "w2t");
  }
  auto stream = at::hip::getCurrentHIPStream();
  nerrf::launch_proj_dgrad_dual(
      a1.data_ptr(), dual ? a2.data_ptr() : nullptr, w1t.data_ptr(),
      dual ? w2t.data_ptr() : nullptr, c.data_ptr(), a1.size(0),
      stream.stream());
}

// Dual-direction input-projection weight grads: dW_d = g_d^T @ x for both
// directions in one launch (transposed LDS tiles, f32 atomic partials).
std::vector<torch::Tensor> proj_wgrad(torch::Tensor g1, torch::Tensor g2,
                                      torch::Tensor x, long n_mchunks) {
  // g1/g2 may be column slabs of one [M, 2048] cat-layout grad (rows
  // contiguous, shared row stride)
  const long g_stride = row_stride_checked(g1, "g1");
  check_gpu_contig(x, "x");
  TORCH_CHECK(g1.scalar_type() == torch::kBFloat16, "proj_wgrad is bf16-only");
  TORCH_CHECK(g1.size(1) == 1024 && x.size(1) == 512,
              "proj_wgrad requires g [M,1024], x [M,512]");
  const bool dual = g2.numel() > 0;
  if (dual)
    TORCH_CHECK(row_stride_checked(g2, "g2") == g_stride,
                "g1/g2 must share a row stride");
  auto dw1 = torch::zeros({1024, 512}, x.options().dtype(torch::kFloat32));
  auto dw2 = dual ? torch::zeros({1024, 512}, x.options().dtype(torch::kFloat32))
                  : torch::empty({0}, x.options().dtype(torch::kFloat32));
  auto stream = at::hip::getCurrentHIPStream();
  nerrf::launch_proj_wgrad(g1.data_ptr(), dual ? g2.data_ptr() : nullptr,
                           x.data_ptr(), dw1.data_ptr<float>(),
                           dual ? dw2.data_ptr<float>() : nullptr, g1.size(0),
                           g_stride, (int)n_mchunks, stream.stream());
  return {dw1, dw2};
}

// GPU delta compaction: event columns -> per-node accumulators -> x [M, 32].
torch::Tensor event_features(torch::Tensor ev_file, torch::Tensor ev_proc,
                             torch::Tensor syscall_id, torch::Tensor nbytes,
                             torch::Tensor ts_ms, long m_nodes,
                             torch::Tensor in_deg, torch::Tensor out_deg,
                             torch::Tensor peer, torch::Tensor flags,
                             torch::Tensor node_kind, double span_s) {
  for (auto* t : {&ev_file, &ev_proc, &syscall_id, &nbytes, &ts_ms, &in_deg,
                  &out_deg, &peer, &flags, &node_kind})
    check_gpu_contig(*t, "event_features arg");
  const long n_events = ev_file.numel();
  auto opts_f = nbytes.options().dtype(torch::kFloat32);
  auto opts_i = nbytes.options().dtype(torch::kInt32);
  auto acc = torch::zeros({m_nodes, 13}, opts_f);
  auto t_first = torch::full({m_nodes}, (long)INT_MAX, opts_i);
  auto t_last = torch::full({m_nodes}, (long)INT_MIN, opts_i);
  auto x = torch::empty({m_nodes, 32}, opts_f);
  auto stream = at::hip::getCurrentHIPStream();
  nerrf::launch_event_scatter(
      ev_file.data_ptr<long>(), ev_proc.data_ptr<long>(),
      syscall_id.data_ptr<signed char>(), nbytes.data_ptr<float>(),
      ts_ms.data_ptr<int>(), acc.data_ptr<float>(), t_first.data_ptr<int>(),
      t_last.data_ptr<int>(), n_events, stream.stream());
  nerrf::launch_feature_assemble(
      acc.data_ptr<float>(), t_first.data_ptr<int>(), t_last.data_ptr<int>(),
      in_deg.data_ptr<float>(), out_deg.data_ptr<float>(),
      peer.data_ptr<float>(), flags.data_ptr<unsigned char>(),
      node_kind.data_ptr<signed char>(), x.data_ptr<float>(), (float)span_s,
      (int)m_nodes, stream.stream());
  return x;
}

// Fused GraphSAGE-T layer forward (inference): gather + dual MFMA GEMM +
// GELU + LayerNorm + residual in one launch.  bf16, D=128 only.
torch::Tensor sage_layer_fwd(torch::Tensor h, torch::Tensor nbr_idx,
                             torch::Tensor nbr_w, torch::Tensor w_self,
                             torch::Tensor w_nbr, torch::Tensor bias,
                             torch::Tensor gamma, torch::Tensor beta) {
  for (auto* t : {&h, &w_self, &w_nbr}) {
    check_gpu_contig(*t, "sage arg");
    TORCH_CHECK(t->scalar_type() == torch::kBFloat16, "sage_layer_fwd is bf16-only");
  }
  check_gpu_contig(nbr_idx, "nbr_idx");
  TORCH_CHECK(h.size(1) == 128 && w_self.size(0) == 128 && w_self.size(1) == 128 &&
                  w_nbr.size(0) == 128 && w_nbr.size(1) == 128,
              "sage_layer_fwd requires D=128");
  const int n = h.size(0);
  const int k = nbr_idx.size(1);
  TORCH_CHECK(k <= 64, "fanout must be <= 64");
  auto wf = nbr_w.scalar_type() == torch::kFloat32 ? nbr_w.contiguous()
                                                   : nbr_w.to(torch::kFloat32).contiguous();
  auto bc = bias.contiguous().to(torch::kBFloat16);
  auto gc = gamma.contiguous().to(torch::kBFloat16);
  auto be = beta.contiguous().to(torch::kBFloat16);
  auto out = torch::empty_like(h);
  auto stream = at::hip::getCurrentHIPStream();
  nerrf::launch_sage_layer_fwd(h.data_ptr(), nbr_idx.data_ptr<long>(),
                               wf.data_ptr<float>(), w_self.data_ptr(),
                               w_nbr.data_ptr(), bc.data_ptr(), gc.data_ptr(),
                               be.data_ptr(), out.data_ptr(), n, k,
                               stream.stream());
  return out;
}

// Fused GraphSAGE-T edge head forward (inference): gather both endpoints,
// build [h_s*h_d, |h_s-h_d|, ew, ets], Linear(258->64) + GELU + Linear(64->1)
// in one launch.  bf16, hidden=128, edge_head_hidden=64 only.  w1_main is
// W1[:, :256] contiguous, w1_tail is W1[:, 256:258] in fp32.  src/dst must lie
// in [0, N): the kernel does not check them.
torch::Tensor edge_head_fwd(torch::Tensor h, torch::Tensor src,
                            torch::Tensor dst, torch::Tensor ew,
                            torch::Tensor ets, torch::Tensor w1_main,
                            torch::Tensor w1_tail, torch::Tensor b1,
                            torch::Tensor w2, torch::Tensor b2) {
  const torch::Tensor* all[] = {&h, &src, &dst, &ew, &ets, &w1_main,
                                &w1_tail, &b1, &w2, &b2};
  const char* names[] = {"h", "src", "dst", "ew", "ets", "w1_main",
                         "w1_tail", "b1", "w2", "b2"};
  for (int i = 0; i < 10; ++i) {
    check_gpu_contig(*all[i], names[i]);
    TORCH_CHECK(all[i]->device() == h.device(), names[i],
                " must be on the same device as h");
  }
  for (auto* t : {&h, &w1_main, &b1, &w2, &b2})
    TORCH_CHECK(t->scalar_type() == torch::kBFloat16,
                "edge_head_fwd: h, w1_main, b1, w2, b2 must be bf16");
  TORCH_CHECK(src.scalar_type() == torch::kInt64 &&
                  dst.scalar_type() == torch::kInt64,
              "edge_head_fwd: src/dst must be int64");
  TORCH_CHECK(ew.scalar_type() == torch::kFloat32 &&
                  ets.scalar_type() == torch::kFloat32 &&
                  w1_tail.scalar_type() == torch::kFloat32,
              "edge_head_fwd: ew, ets, w1_tail must be fp32");
  TORCH_CHECK(h.dim() == 2 && h.size(1) == 128,
              "edge_head_fwd requires hidden=128 (h is [N, 128])");
  TORCH_CHECK(w1_main.dim() == 2 && w1_main.size(0) == 64 &&
                  w1_main.size(1) == 256 && w1_tail.dim() == 2 &&
                  w1_tail.size(0) == 64 && w1_tail.size(1) == 2 &&
                  b1.numel() == 64 && w2.numel() == 64 && b2.numel() == 1,
              "edge_head_fwd requires edge_head_hidden=64: w1_main [64,256], "
              "w1_tail [64,2], b1 [64], w2 [64], b2 [1]");
  const long n_edges = src.numel();
  TORCH_CHECK(src.dim() == 1 && dst.dim() == 1 && ew.dim() == 1 &&
                  ets.dim() == 1 && dst.numel() == n_edges &&
                  ew.numel() == n_edges && ets.numel() == n_edges,
              "edge_head_fwd: src, dst, ew, ets must all be [E]");
  TORCH_CHECK(n_edges == 0 || h.size(0) > 0,
              "edge_head_fwd: edges over an empty node set");
  check_vec_base(h, true, "h");
  check_vec_base(w1_main, true, "w1_main");
  auto out = torch::empty({n_edges}, h.options().dtype(torch::kFloat32));
  if (n_edges == 0) return out;
  auto stream = at::hip::getCurrentHIPStream();
  nerrf::launch_edge_head_fwd(
      h.data_ptr(), src.data_ptr<long>(), dst.data_ptr<long>(),
      ew.data_ptr<float>(), ets.data_ptr<float>(), w1_main.data_ptr(),
      w1_tail.data_ptr<float>(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(),
      out.data_ptr<float>(), n_edges, stream.stream());
  const hipError_t launch_err = hipGetLastError();
  TORCH_CHECK(launch_err == hipSuccess, "edge_head_fwd launch failed: ",
              hipGetErrorString(launch_err));
  return out;
}

// Per-file edge attribution: for each file node, the process whose wanted-
// direction edge (write: proc -> file, read: file -> proc) has the highest
// logit, that logit, and the count of such edges with logit >= thr_logit.
// Nodes [0, n_files) are files, [n_files, n_nodes) processes.  Edges with an
// endpoint outside [0, n_nodes) are skipped by the kernel, not read through.
// Returns (culprit [n_files] int64, -1 = none; best_logit [n_files] fp32,
// -inf = none; n_hot [n_files] int32).  No host synchronisation.
std::vector<torch::Tensor> edge_attr(torch::Tensor logit, torch::Tensor src,
                                     torch::Tensor dst, long n_files,
                                     long n_nodes, bool want_write,
                                     double thr_logit) {
  const torch::Tensor* all[] = {&logit, &src, &dst};
  const char* names[] = {"logit", "src", "dst"};
  for (int i = 0; i < 3; ++i) {
    check_gpu_contig(*all[i], names[i]);
    TORCH_CHECK(all[i]->device() == logit.device(), names[i],
                " must be on the same device as logit");
  }
  TORCH_CHECK(logit.scalar_type() == torch::kFloat32,
              "edge_attr: logit must be fp32");
  TORCH_CHECK(src.scalar_type() == torch::kInt64 &&
                  dst.scalar_type() == torch::kInt64,
              "edge_attr: src/dst must be int64");
  const long n_edges = logit.numel();
  TORCH_CHECK(logit.dim() == 1 && src.dim() == 1 && dst.dim() == 1 &&
                  src.numel() == n_edges && dst.numel() == n_edges,
              "edge_attr: logit, src, dst must all be [E]");
  TORCH_CHECK(n_files >= 0 && n_files <= n_nodes,
              "edge_attr: need 0 <= n_files <= n_nodes, got n_files=", n_files,
              " n_nodes=", n_nodes);
  TORCH_CHECK(n_nodes - n_files < (1L << 32),
              "edge_attr: at most 2^32 - 1 process nodes");
  auto opts = logit.options();
  auto n_hot = torch::zeros({n_files}, opts.dtype(torch::kInt32));
  if (n_edges == 0 || n_files == 0) {
    return {torch::full({n_files}, -1L, opts.dtype(torch::kInt64)),
            torch::full({n_files}, -std::numeric_limits<float>::infinity(),
                        opts.dtype(torch::kFloat32)),
            n_hot};
  }
  // packed (orderable logit, inverted process index) keys; zero = no edge
  auto best = torch::zeros({n_files}, opts.dtype(torch::kInt64));
  auto culprit = torch::empty({n_files}, opts.dtype(torch::kInt64));
  auto best_logit = torch::empty({n_files}, opts.dtype(torch::kFloat32));
  auto stream = at::hip::getCurrentHIPStream();
  nerrf::launch_edge_attr(
      logit.data_ptr<float>(), src.data_ptr<long>(), dst.data_ptr<long>(),
      reinterpret_cast<unsigned long long*>(best.data_ptr<long>()),
      n_hot.data_ptr<int>(), culprit.data_ptr<long>(),
      best_logit.data_ptr<float>(), n_edges, n_files, n_nodes, want_write,
      static_cast<float>(thr_logit), stream.stream());
  const hipError_t launch_err = hipGetLastError();
  TORCH_CHECK(launch_err == hipSuccess, "edge_attr launch failed: ",
              hipGetErrorString(launch_err));
  return {culprit, best_logit, n_hot};
}

// Fused GraphSAGE training-layer tail: y = h + LN(dropout(GELU(zs+zn)))*g+b
std::vector<torch::Tensor> sage_ln_act_fwd(torch::Tensor h, torch::Tensor zs,
                                           torch::Tensor zn, torch::Tensor gamma,
                                           torch::Tensor beta, double drop_p,
                                           long seed, bool want_mask) {
  for (auto* t : {&h, &zs, &zn}) {
    check_gpu_contig(*t, "sage_ln_act arg");
    TORCH_CHECK(t->scalar_type() == torch::kBFloat16, "sage_ln_act is bf16-only");
    TORCH_CHECK(t->size(1) == 128, "sage_ln_act requires D=128");
  }
  const long n = h.size(0);
  auto gc = gamma.contiguous().to(torch::kBFloat16);
  auto bc = beta.contiguous().to(torch::kBFloat16);
  auto y = torch::empty_like(h);
  auto s_save = torch::empty_like(h);
  auto stats = torch::empty({n, 2}, h.options().dtype(torch::kFloat32));
  torch::Tensor mask = want_mask
      ? torch::zeros({n, 128}, h.options().dtype(torch::kUInt8))
      : torch::empty({0}, h.options().dtype(torch::kUInt8));
  auto stream = at::hip::getCurrentHIPStream();
  nerrf::launch_sage_ln_act_fwd(
      h.data_ptr(), zs.data_ptr(), zn.data_ptr(), gc.data_ptr(), bc.data_ptr(),
      y.data_ptr(), s_save.data_ptr(), stats.data_ptr<float>(),
      want_mask ? mask.data_ptr<unsigned char>() : nullptr, n, (float)drop_p,
      (unsigned)seed, stream.stream());
  return {y, s_save, stats, mask};
}

std::vector<torch::Tensor> sage_ln_act_bwd(torch::Tensor dy, torch::Tensor s_save,
                                           torch::Tensor stats, torch::Tensor gamma,
                                           double drop_p, long seed) {
  check_gpu_contig(dy, "dy");
  check_gpu_contig(s_save, "s_save");
  check_gpu_contig(stats, "stats");
  const long n = dy.size(0);
  auto gc = gamma.contiguous().to(torch::kBFloat16);
  auto dz = torch::empty_like(dy);
  const long grid = (n + 7) / 8;
  auto dg_part = torch::empty({grid, 128}, dy.options().dtype(torch::kFloat32));
  auto db_part = torch::empty({grid, 128}, dy.options().dtype(torch::kFloat32));
  auto stream = at::hip::getCurrentHIPStream();
  nerrf::launch_sage_ln_act_bwd(
      dy.data_ptr(), s_save.data_ptr(), stats.data_ptr<float>(), gc.data_ptr(),
      dz.data_ptr(), dg_part.data_ptr<float>(), db_part.data_ptr<float>(), n,
      (float)drop_p, (unsigned)seed, stream.stream());
  return {dz, dg_part.sum(0), db_part.sum(0)};
}

nerrf::PlannerParamsDev params_from_dict(const pybind11::dict& d) {
  nerrf::PlannerParamsDev p;
  p.n_groups = d["n_groups"].cast<int>();
  p.n_actions = p.n_groups + 3;  // STOP, KILL, RESTORE, revert g
  p.max_depth = d["max_depth"].cast<int>();
  p.sims_per_tree = d["sims_per_tree"].cast<int>();
  p.downtime_weight = d["downtime_weight"].cast<float>();
  p.revert_time_s = d["revert_time_s"].cast<float>();
  p.kill_time_s = d["kill_time_s"].cast<float>();
  p.fp_weight = d["fp_weight"].cast<float>();
  p.attack_rate_mbps = d["attack_rate_mbps"].cast<float>();
  p.horizon_s = d["horizon_s"].cast<float>();
  p.restore_time_s = d["restore_time_s"].cast<float>();
  p.restore_loss_mb = d["restore_loss_mb"].cast<float>();
  p.ucb_c = d["ucb_c"].cast<float>();
  p.seed = d["seed"].cast<unsigned>();
  TORCH_CHECK(p.n_groups <= 16, "n_groups must be <= 16");
  TORCH_CHECK(p.max_depth <= 16, "max_depth must be <= 16");
  return p;
}

std::vector<torch::Tensor> mcts_search(torch::Tensor gscore, torch::Tensor gmb,
                                       torch::Tensor gfiles, double proc_score,
                                       double remaining_clean_mb,
                                       pybind11::dict param_dict, long n_trees) {
  auto p = params_from_dict(param_dict);
  check_gpu_contig(gscore, "gscore");
  check_gpu_contig(gmb, "gmb");
  check_gpu_contig(gfiles, "gfiles");
  const int cap = p.sims_per_tree * p.max_depth + 2;
  auto opts_i = gscore.options().dtype(torch::kInt32);
  auto opts_f = gscore.options().dtype(torch::kFloat32);
  auto arena_i = torch::empty({n_trees, (long)(3 * cap + cap * p.n_actions)}, opts_i);
  auto arena_f = torch::empty({n_trees, (long)cap}, opts_f);
  auto root_visits = torch::zeros({n_trees, (long)p.n_actions}, opts_i);
  auto root_value = torch::zeros({n_trees, (long)p.n_actions}, opts_f);
  auto stream = at::hip::getCurrentHIPStream();
  nerrf::launch_mcts(gscore.data_ptr<float>(), gmb.data_ptr<float>(),
                     gfiles.data_ptr<float>(), (float)proc_score,
                     (float)remaining_clean_mb, p, (int)n_trees, cap,
                     arena_i.data_ptr<int>(), arena_f.data_ptr<float>(),
                     root_visits.data_ptr<int>(), root_value.data_ptr<float>(),
                     stream.stream());
  return {root_visits, root_value};
}

torch::Tensor mcts_eval_plans(torch::Tensor gscore, torch::Tensor gmb,
                              torch::Tensor gfiles, double proc_score,
                              double remaining_clean_mb,
                              pybind11::dict param_dict, torch::Tensor plans) {
  auto p = params_from_dict(param_dict);
  check_gpu_contig(plans, "plans");
  TORCH_CHECK(plans.scalar_type() == torch::kInt32, "plans must be int32");
  const int n_plans = plans.size(0);
  const int plan_len = plans.size(1);
  auto out = torch::empty({(long)n_plans}, gscore.options().dtype(torch::kFloat32));
  auto stream = at::hip::getCurrentHIPStream();
  nerrf::launch_eval_plans(gscore.data_ptr<float>(), gmb.data_ptr<float>(),
                           gfiles.data_ptr<float>(), (float)proc_score,
                           (float)remaining_clean_mb, p, plans.data_ptr<int>(),
                           n_plans, plan_len, out.data_ptr<float>(),
                           stream.stream());
  return out;
}

// Exhaustive plan oracle over a batch of S states (plan_oracle.hip).
// Returns CPU tensors, one row per state and one slot per first action
// (slot 0 = STOP, the empty plan; slot a = best plan starting with action a):
//   [0] reward  f32 [S, n+1]  eval_plan's value of the winner (== mcts_eval_plans)
//   [1] len     i32 [S, n+1]
//   [2] plan    i32 [S, n+1, 16]  STOP-padded
//   [3] meta    i64 [2]       prefix length L, prefixes per state
std::vector<torch::Tensor> plan_oracle_search(
    torch::Tensor gscore, torch::Tensor gmb, torch::Tensor gfiles,
    torch::Tensor proc, torch::Tensor clean, pybind11::dict param_dict,
    long prefix_len) {
  auto p = params_from_dict(param_dict);
  const torch::Tensor* ins[] = {&gscore, &gmb, &gfiles, &proc, &clean};
  const char* names[] = {"gscore", "gmb", "gfiles", "proc", "clean"};
  for (int i = 0; i < 5; ++i) {
    check_gpu_contig(*ins[i], names[i]);
    TORCH_CHECK(ins[i]->scalar_type() == torch::kFloat32, names[i],
                " must be float32");
  }
  TORCH_CHECK(gscore.dim() == 2, "gscore must be [S, G]");
  const long S = gscore.size(0);
  const int G = p.n_groups;
  TORCH_CHECK(S >= 1 && S <= (1 << 20), "need 1 <= S <= 2^20 states");
  TORCH_CHECK(G >= 1, "n_groups must be >= 1");
  TORCH_CHECK(p.max_depth >= 1, "max_depth must be >= 1");
  TORCH_CHECK(gscore.size(1) == G && gmb.sizes() == gscore.sizes() &&
                  gfiles.sizes() == gscore.sizes(),
              "gscore/gmb/gfiles must all be [S, n_groups]");
  TORCH_CHECK(proc.dim() == 1 && proc.size(0) == S && clean.dim() == 1 &&
                  clean.size(0) == S,
              "proc/clean must be [S]");
  const int n = G + 2;  // non-STOP actions
  const int depth_lim = std::min(p.max_depth, n);
  const long kMaxPrefix = 1L << 22;
  int L = 1;
  long n_prefix = n;
  if (prefix_len > 0) {
    TORCH_CHECK(prefix_len <= depth_lim, "prefix_len must be <= min(max_depth, n)");
    for (L = 1; L < prefix_len; ++L) n_prefix *= (n - L);
    TORCH_CHECK(n_prefix <= kMaxPrefix, "prefix_len gives too many prefixes");
  } else {
    // enough work items to fill the device, but leave the search some depth
    const int l_max = std::max(1, depth_lim - 3);
    const long target = 65536;
    while (L < l_max && S * n_prefix < target &&
           n_prefix * (n - L) <= kMaxPrefix) {
      n_prefix *= (n - L);
      ++L;
    }
  }
  TORCH_CHECK(S * n_prefix <= (1L << 26),
              "too many work items (states x prefixes); lower prefix_len or "
              "split the batch");

  auto opts_f = gscore.options().dtype(torch::kFloat32);
  auto opts_i = gscore.options().dtype(torch::kInt32);
  auto item_reward = torch::empty({S, n_prefix}, opts_f);
  auto item_len = torch::empty({S, n_prefix}, opts_i);
  auto item_plan = torch::empty({S, n_prefix, 6}, opts_i);
  auto stream = at::hip::getCurrentHIPStream();
  nerrf::launch_plan_oracle(
      gscore.data_ptr<float>(), gmb.data_ptr<float>(), gfiles.data_ptr<float>(),
      proc.data_ptr<float>(), clean.data_ptr<float>(), p, (int)S, L,
      (int)n_prefix, item_reward.data_ptr<float>(), item_len.data_ptr<int>(),
      reinterpret_cast<unsigned*>(item_plan.data_ptr<int>()), stream.stream());
  const hipError_t launch_err = hipGetLastError();
  TORCH_CHECK(launch_err == hipSuccess, "plan oracle launch failed: ",
              hipGetErrorString(launch_err));

  // ---- reduce the prefix winners by first action (host; not hot) ----
  auto h_reward = item_reward.cpu();
  auto h_len = item_len.cpu();
  auto h_plan = item_plan.cpu();
  auto h_proc = proc.cpu();
  auto h_clean = clean.cpu();
  const float* hr = h_reward.data_ptr<float>();
  const int* hl = h_len.data_ptr<int>();
  const unsigned* hp = reinterpret_cast<const unsigned*>(h_plan.data_ptr<int>());
  auto cpu_i = torch::TensorOptions().dtype(torch::kInt32);
  auto win_len = torch::zeros({S, (long)n + 1}, cpu_i);
  auto win_plan = torch::zeros({S, (long)n + 1, 16}, cpu_i);
  int* wl = win_len.data_ptr<int>();
  int* wp = win_plan.data_ptr<int>();
  auto field = [](const unsigned* w, int i) {
    return (int)((w[i / 6] >> (5 * (i % 6))) & 31u);
  };
  for (long s = 0; s < S; ++s) {
    std::vector<long> best(n + 1, -1);
    for (long i = 0; i < n_prefix; ++i) {
      const long o = s * n_prefix + i;
      const int len = hl[o];
      TORCH_CHECK(len >= 1 && len <= depth_lim,
                  "plan oracle: no finite reward under a prefix "
                  "(non-finite planner inputs?)");
      const int a0 = field(hp + o * 6, 0);
      TORCH_CHECK(a0 >= 1 && a0 <= n, "plan oracle: corrupt winner");
      const long b = best[a0];
      // items are in lexicographic prefix order: an equal (reward, len)
      // keeps the earlier one
      if (b < 0 || hr[o] > hr[b] || (hr[o] == hr[b] && len < hl[b])) best[a0] = o;
    }
    for (int a = 1; a <= n; ++a) {
      const long o = best[a];
      TORCH_CHECK(o >= 0, "plan oracle: first action without a winner");
      const long slot = s * (n + 1) + a;
      const int len = hl[o];
      wl[slot] = len;
      for (int i = 0; i < len; ++i) {
        const int act = (i < L) ? field(hp + o * 6, i) : field(hp + o * 6 + 3, i - L);
        TORCH_CHECK(act >= 1 && act <= n, "plan oracle: corrupt winner");
        wp[slot * 16 + i] = act;
      }
    }
  }

  // ---- reported rewards: eval_plan on the winners ----
  auto d_plans = win_plan.to(gscore.device());
  auto d_reward = torch::empty({S, (long)n + 1}, opts_f);
  const float* pproc = h_proc.data_ptr<float>();
  const float* pclean = h_clean.data_ptr<float>();
  for (long s = 0; s < S; ++s) {
    nerrf::launch_eval_plans(
        gscore.data_ptr<float>() + s * G, gmb.data_ptr<float>() + s * G,
        gfiles.data_ptr<float>() + s * G, pproc[s], pclean[s], p,
        d_plans.data_ptr<int>() + s * (n + 1) * 16, n + 1, 16,
        d_reward.data_ptr<float>() + s * (n + 1), stream.stream());
  }
  auto win_reward = d_reward.cpu();
  auto meta = torch::zeros({2}, torch::TensorOptions().dtype(torch::kInt64));
  meta.data_ptr<int64_t>()[0] = L;
  meta.data_ptr<int64_t>()[1] = n_prefix;
  return {win_reward, win_len, win_plan, meta};
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("sage_ln_act_fwd", &sage_ln_act_fwd,
        "fused GNN layer tail fwd (add+GELU+dropout+LN+residual)");
  m.def("sage_ln_act_bwd", &sage_ln_act_bwd, "fused GNN layer tail bwd");
  m.def("sage_layer_fwd", &sage_layer_fwd,
        "fused GraphSAGE-T layer forward (MFMA, inference)");
  m.def("edge_head_fwd", &edge_head_fwd,
        "fused GraphSAGE-T edge head forward (MFMA, inference) -> fp32 [E]");
  m.def("edge_attr", &edge_attr,
        "per-file best edge: (culprit [F] int64, best_logit [F] fp32, "
        "n_hot [F] int32)");
  m.def("event_features", &event_features,
        "GPU delta compaction: events -> per-node feature matrix");
  m.def("mcts_search", &mcts_search, "batched root-parallel MCTS");
  m.def("mcts_eval_plans", &mcts_eval_plans, "batch plan reward evaluation");
  m.def("plan_oracle_search", &plan_oracle_search,
        "exhaustive best plan per first action over a batch of states",
        pybind11::arg("gscore"), pybind11::arg("gmb"), pybind11::arg("gfiles"),
        pybind11::arg("proc"), pybind11::arg("clean"), pybind11::arg("params"),
        pybind11::arg("prefix_len") = 0);
  m.def("gather_mean_fwd", &gather_mean_fwd, "weighted neighbor gather-mean");
  m.def("gather_mean_bwd", &gather_mean_bwd, "gather-mean backward");
  m.def("gather_mean_bwd_csr", &gather_mean_bwd_csr,
        "deterministic gather-mean backward over reverse CSR");
  m.def("lstm_pointwise_fwd", &lstm_pointwise_fwd,
        "fused LSTM gate pointwise fwd", py::arg("hg"), py::arg("xg"),
        py::arg("bias"), py::arg("c_prev"), py::arg("h_prev"), py::arg("mask"),
        py::arg("h_out"), py::arg("c_out"), py::arg("gates_act"),
        py::arg("prev_rows") = -1);
  m.def("lstm_rec_fwd", &lstm_rec_fwd,
        "fused recurrent GEMM + LSTM pointwise fwd (bf16, H=256)");
  m.def("lstm_rec_bwd", &lstm_rec_bwd,
        "fused LSTM gate grads + grad_h GEMM bwd (bf16, H=256)");
  m.def("rec_gemm_fwd", &rec_gemm_fwd,
        "recurrent-step GEMM [M,256]x[1024,256]^T (bf16, strided rows)");
  m.def("rec_gemm_dgrad", &rec_gemm_dgrad,
        "recurrence backward dgrad [M,1024]x[256,1024]^T + addend (bf16)");
  m.def("proj_fwd_dual", &proj_fwd_dual,
        "dual-direction LSTM input projection (A read once)");
  m.def("proj_dgrad_dual", &proj_dgrad_dual,
        "dual-direction input-projection dgrad (summed)");
  m.def("proj_wgrad", &proj_wgrad,
        "dual-direction input-projection weight grads (f32 partials)");
  m.def("lstm_step_fused", &lstm_step_fused, "fully-fused MFMA LSTM step (bf16, H=256)");
  m.def("lstm_pointwise_bwd", &lstm_pointwise_bwd,
        "fused LSTM gate pointwise bwd", py::arg("grad_h"),
        py::arg("grad_out_t"), py::arg("grad_c"), py::arg("gates_act"),
        py::arg("c_prev"), py::arg("mask"), py::arg("grad_gates"),
        py::arg("grad_c_prev"), py::arg("grad_h_pass"), py::arg("bias_accum"),
        py::arg("in_rows") = -1, py::arg("prev_rows") = -1);
}
