// Torch bindings for the wva_amd MI355X (gfx950) kernels.
//
// Built in-tree via torch.utils.cpp_extension (PYTORCH_ROCM_ARCH=gfx950).
// The kernels' host entry points are declared in launch.h, which the .hip
// files include too; nothing is re-declared here. Each kernel family has one
// implementation below (decode attention, KV append, skinny linear, prefill
// operands) behind its contiguous/paged or bf16/fp8 bindings, so a check or
// a launch argument is edited in one place.

#include <torch/extension.h>
#include <c10/hip/HIPStream.h>

#include <string>

#include "launch.h"

namespace {

hipStream_t current_stream() {
  return c10::hip::getCurrentHIPStream().stream();
}

void check_bf16_contig(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be on GPU");
  TORCH_CHECK(t.scalar_type() == torch::kBFloat16, name, " must be bf16");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
}

void check_i32_contig(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be on GPU");
  TORCH_CHECK(t.scalar_type() == torch::kInt32, name, " must be int32");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
}

// A K/V cache (or paged pool) pair: both on the GPU and contiguous, the same
// dtype, bf16 or fp8 e4m3 (torch float8_e4m3fn), and the same shape. Returns
// true when the pair is fp8.
bool check_kv_pair(const torch::Tensor& k, const torch::Tensor& v) {
  TORCH_CHECK(k.is_cuda() && v.is_cuda(), "k/v cache must be on GPU");
  TORCH_CHECK(k.is_contiguous() && v.is_contiguous(),
              "k/v cache must be contiguous");
  const bool fp8 = k.scalar_type() == at::kFloat8_e4m3fn;
  TORCH_CHECK(fp8 || k.scalar_type() == torch::kBFloat16,
              "k/v cache must be bf16 or float8_e4m3fn");
  TORCH_CHECK(v.scalar_type() == k.scalar_type(), "k/v cache dtype mismatch");
  TORCH_CHECK(v.sizes() == k.sizes(), "k/v cache shape mismatch");
  return fp8;
}

// Paged operands shared by the decode attention and KV append ops: k_pages
// (and v_pages, see check_kv_pair) are [num_blocks, Hk, block_size, 128],
// block_tables [B, max_blocks]. Returns the launch descriptor.
PagedKV check_paged_pool(const torch::Tensor& k_pages,
                         const torch::Tensor& block_tables, int64_t batch) {
  TORCH_CHECK(k_pages.dim() == 4 && k_pages.size(3) == 128,
              "k_pages must be [num_blocks, Hk, block_size, 128]");
  const int64_t num_blocks = k_pages.size(0);
  const int64_t block_size = k_pages.size(2);
  TORCH_CHECK(num_blocks >= 1, "the pool needs at least one block");
  TORCH_CHECK(block_size == 16 || block_size == 32 || block_size == 64,
              "block_size must be 16, 32 or 64, got ", block_size);
  check_i32_contig(block_tables, "block_tables");
  TORCH_CHECK(block_tables.dim() == 2 && block_tables.size(0) == batch &&
                  block_tables.size(1) >= 1,
              "block_tables must be [B, max_blocks]");
  // page offsets are formed in 64-bit; pool rows, table entries and
  // positions stay in int32
  TORCH_CHECK(num_blocks * k_pages.size(1) * block_size < (1L << 31),
              "num_blocks * Hk * block_size must be below 2^31");
  TORCH_CHECK(block_tables.size(1) * block_size < (1L << 31) &&
                  batch * block_tables.size(1) < (1L << 31),
              "block_tables too large");
  return PagedKV{block_tables.data_ptr<int>(), (int)block_tables.size(1),
                 block_size == 16 ? 4 : block_size == 32 ? 5 : 6,
                 (int)num_blocks};
}

// out = rmsnorm(input [+ residual]) * weight; when residual is given it is
// updated in place to (input + residual).
torch::Tensor rmsnorm(torch::Tensor input, torch::Tensor weight,
                      c10::optional<torch::Tensor> residual, double eps) {
  check_bf16_contig(input, "input");
  check_bf16_contig(weight, "weight");
  const int hidden = input.size(-1);
  TORCH_CHECK(hidden % 8 == 0, "hidden must be a multiple of 8");
  TORCH_CHECK(weight.numel() == hidden, "weight size mismatch");
  auto out = torch::empty_like(input);
  const void* res_ptr = nullptr;
  void* res_out_ptr = nullptr;
  if (residual.has_value()) {
    check_bf16_contig(residual.value(), "residual");
    TORCH_CHECK(residual->sizes() == input.sizes(), "residual shape mismatch");
    res_ptr = residual->data_ptr();
    res_out_ptr = residual->data_ptr();  // in-place fold
  }
  // no rows (or hidden == 0): a zero-sized grid is an invalid launch
  if (input.numel() == 0) return out;
  const long rows = input.numel() / hidden;
  launch_rmsnorm(out.data_ptr(), res_out_ptr, input.data_ptr(), res_ptr,
                 weight.data_ptr(), (float)eps, (int)rows, hidden,
                 current_stream());
  return out;
}

// In-place NeoX-style RoPE on q [T,Hq,D] and k [T,Hk,D] at positions [T].
void rope(torch::Tensor q, torch::Tensor k, torch::Tensor positions,
          double theta) {
  check_bf16_contig(q, "q");
  check_bf16_contig(k, "k");
  check_i32_contig(positions, "positions");
  TORCH_CHECK(q.dim() == 3 && k.dim() == 3, "q/k must be [T, H, D]");
  const int tokens = q.size(0);
  const int num_q_heads = q.size(1);
  const int num_k_heads = k.size(1);
  const int head_dim = q.size(2);
  TORCH_CHECK(k.size(0) == tokens && k.size(2) == head_dim, "q/k mismatch");
  TORCH_CHECK(head_dim % 2 == 0, "head_dim must be even");
  launch_rope(q.data_ptr(), k.data_ptr(), positions.data_ptr<int>(), tokens,
              num_q_heads, num_k_heads, head_dim, (float)theta,
              current_stream());
}

torch::Tensor silu_mul(torch::Tensor gate, torch::Tensor up) {
  check_bf16_contig(gate, "gate");
  check_bf16_contig(up, "up");
  TORCH_CHECK(gate.sizes() == up.sizes(), "gate/up shape mismatch");
  TORCH_CHECK(gate.numel() % 2 == 0, "numel must be even");
  auto out = torch::empty_like(gate);
  launch_silu_mul(out.data_ptr(), gate.data_ptr(), up.data_ptr(),
                  (long)gate.numel(), current_stream());
  return out;
}

// Decode fast path: strided qkv row → RoPE'd q_out + cache append at
// positions[b]. Contiguous caches are [>= B, Hk, S, D]. With block_tables the
// caches are a paged pool and the K/V row of sequence b goes to page
// block_tables[b, pos / block_size], row pos % block_size; a position past
// the table or an entry outside [0, num_blocks) skips the K/V stores
// (csrc/rope.hip paged_row_offset).
torch::Tensor rope_append_kv_impl(
    const torch::Tensor& qkv, const torch::Tensor& k_cache,
    const torch::Tensor& v_cache,
    const c10::optional<torch::Tensor>& block_tables,
    const torch::Tensor& positions, int64_t num_q_heads, int64_t num_kv_heads,
    double theta) {
  check_bf16_contig(qkv, "qkv");
  const bool kv_fp8 = check_kv_pair(k_cache, v_cache);
  check_i32_contig(positions, "positions");
  TORCH_CHECK(qkv.dim() == 2, "qkv must be [B, (Hq+2Hk)*D]");
  const int batch = qkv.size(0);
  TORCH_CHECK(positions.dim() == 1 && positions.size(0) == batch,
              "positions must be [B]");
  PagedKV paged{};
  if (block_tables.has_value()) {
    paged = check_paged_pool(k_cache, *block_tables, batch);
  } else {
    TORCH_CHECK(k_cache.dim() == 4, "k_cache must be [B, Hk, S, D]");
    TORCH_CHECK(k_cache.size(0) >= batch,
                "cache holds fewer than B sequences");
  }
  const int head_dim = k_cache.size(3);
  TORCH_CHECK(k_cache.size(1) == num_kv_heads, "Hk mismatch");
  TORCH_CHECK(qkv.size(1) == (num_q_heads + 2 * num_kv_heads) * head_dim,
              "qkv width mismatch");
  auto q_out = torch::empty({batch, num_q_heads, head_dim}, qkv.options());
  launch_rope_append_kv(qkv.data_ptr(), q_out.data_ptr(), k_cache.data_ptr(),
                        v_cache.data_ptr(), positions.data_ptr<int>(),
                        block_tables.has_value() ? &paged : nullptr, batch,
                        (int)num_q_heads, (int)num_kv_heads, head_dim,
                        (int)k_cache.size(2), (float)theta, kv_fp8 ? 1 : 0,
                        current_stream());
  return q_out;
}

torch::Tensor rope_append_kv(torch::Tensor qkv, torch::Tensor k_cache,
                             torch::Tensor v_cache, torch::Tensor positions,
                             int64_t num_q_heads, int64_t num_kv_heads,
                             double theta) {
  return rope_append_kv_impl(qkv, k_cache, v_cache, c10::nullopt, positions,
                             num_q_heads, num_kv_heads, theta);
}

torch::Tensor rope_append_kv_paged(torch::Tensor qkv, torch::Tensor k_pages,
                                   torch::Tensor v_pages,
                                   torch::Tensor block_tables,
                                   torch::Tensor positions,
                                   int64_t num_q_heads, int64_t num_kv_heads,
                                   double theta) {
  return rope_append_kv_impl(qkv, k_pages, v_pages, block_tables, positions,
                             num_q_heads, num_kv_heads, theta);
}

torch::Tensor silu_mul_fused(torch::Tensor gate_up) {
  check_bf16_contig(gate_up, "gate_up");
  TORCH_CHECK(gate_up.dim() == 2 && gate_up.size(1) % 4 == 0,
              "gate_up must be [rows, 2*inter], inter even");
  const long rows = gate_up.size(0);
  const long inter = gate_up.size(1) / 2;
  auto out = torch::empty({rows, inter}, gate_up.options());
  launch_silu_mul_fused(out.data_ptr(), gate_up.data_ptr(), rows, inter,
                        current_stream());
  return out;
}

// Decode attention kernel choice. Auto is the measured per-shape-class
// dispatch (profiles/attn_v4_ab.txt): v5 (MFMA scores + MFMA PV) wins
// when the PV matrix is well-utilized (G = 8) or the grid is unsplit
// (large batch); v4 (MFMA scores, vector PV) wins for G < 8 with split-KV
// where v5's padded 16-row PV and its third per-tile barrier cost more
// than the VALU sweep it replaces. V4/V5 pin a kernel on any shape, for
// tests and the microbench.
enum class AttnVariant { Auto, V4, V5 };

AttnVariant parse_attn_variant(const std::string& name) {
  TORCH_CHECK(name == "auto" || name == "v4" || name == "v5",
              "variant must be \"auto\", \"v4\" or \"v5\", got \"", name, "\"");
  return name == "v4"   ? AttnVariant::V4
         : name == "v5" ? AttnVariant::V5
                        : AttnVariant::Auto;
}

// GQA decode attention, q/out [B, Hq, 128], context_lens [B]. Contiguous
// caches are [>= B, Hk, S, 128]; with block_tables they are a paged pool
// (check_paged_pool). num_splits absent means the launch heuristic over S,
// or over max_blocks * block_size for a pool. On a pool `auto` applies the
// rule above as it stands; it was measured on the contiguous layout only,
// see docs/mi355x-kernels.md "Paged KV cache" for what pages change.
torch::Tensor decode_attn_impl(
    const torch::Tensor& q, const torch::Tensor& k_cache,
    const torch::Tensor& v_cache,
    const c10::optional<torch::Tensor>& block_tables,
    const torch::Tensor& context_lens, double scale,
    c10::optional<int64_t> forced_splits, const std::string& variant_name) {
  AttnVariant variant = parse_attn_variant(variant_name);
  check_bf16_contig(q, "q");
  const bool kv_fp8 = check_kv_pair(k_cache, v_cache);
  check_i32_contig(context_lens, "context_lens");
  TORCH_CHECK(q.dim() == 3, "q must be [B, Hq, D]");
  const int batch = q.size(0);
  const int num_q_heads = q.size(1);
  const int head_dim = q.size(2);
  TORCH_CHECK(head_dim == 128, "head_dim must be 128 (Llama-3 family)");
  TORCH_CHECK(context_lens.dim() == 1 && context_lens.size(0) == batch,
              "context_lens must be [B]");
  PagedKV paged{};
  int max_seq;
  if (block_tables.has_value()) {
    paged = check_paged_pool(k_cache, *block_tables, batch);
    max_seq = paged.max_blocks << paged.block_shift;
  } else {
    TORCH_CHECK(k_cache.dim() == 4 && k_cache.size(3) == 128,
                "k_cache must be [B, Hk, S, 128] (head-major)");
    TORCH_CHECK(k_cache.size(0) >= batch,
                "cache holds fewer than B sequences");
    max_seq = k_cache.size(2);
  }
  const int num_kv_heads = k_cache.size(1);
  TORCH_CHECK(num_q_heads % num_kv_heads == 0, "Hq must divide by Hk");
  const int G = num_q_heads / num_kv_heads;
  TORCH_CHECK(G <= 8, "GQA group size must be <= 8");
  if (forced_splits.has_value()) {
    TORCH_CHECK(*forced_splits >= 1 && *forced_splits <= 65535,
                "num_splits must be in [1, 65535]");
  }
  const int num_splits =
      forced_splits.has_value()
          ? (int)*forced_splits
          : gqa_decode_attn_num_splits(batch, num_kv_heads, max_seq);
  if (variant == AttnVariant::Auto) {
    variant = (G >= 8 || num_splits == 1) ? AttnVariant::V5 : AttnVariant::V4;
  }
  auto out = torch::empty_like(q);
  torch::Tensor workspace;
  void* ws_ptr = nullptr;
  if (num_splits > 1) {
    workspace = torch::empty(
        {(long)batch * num_kv_heads * G * num_splits * (2 + head_dim)},
        q.options().dtype(torch::kFloat32));
    ws_ptr = workspace.data_ptr();
  }
  launch_gqa_decode_attn(out.data_ptr(), ws_ptr, q.data_ptr(),
                         k_cache.data_ptr(), v_cache.data_ptr(),
                         context_lens.data_ptr<int>(),
                         block_tables.has_value() ? &paged : nullptr, batch,
                         num_q_heads, num_kv_heads, max_seq, num_splits,
                         (float)scale, variant == AttnVariant::V5 ? 5 : 4,
                         kv_fp8 ? 1 : 0, current_stream());
  return out;
}

torch::Tensor gqa_decode_attn(torch::Tensor q, torch::Tensor k_cache,
                              torch::Tensor v_cache,
                              torch::Tensor context_lens, double scale,
                              const std::string& variant,
                              c10::optional<int64_t> num_splits) {
  return decode_attn_impl(q, k_cache, v_cache, c10::nullopt, context_lens,
                          scale, num_splits, variant);
}

torch::Tensor paged_decode_attn(torch::Tensor q, torch::Tensor k_pages,
                                torch::Tensor v_pages,
                                torch::Tensor block_tables,
                                torch::Tensor context_lens, double scale,
                                c10::optional<int64_t> num_splits,
                                const std::string& variant) {
  return decode_attn_impl(q, k_pages, v_pages, block_tables, context_lens,
                          scale, num_splits, variant);
}

int64_t gqa_decode_attn_splits(int64_t batch, int64_t num_kv_heads,
                               int64_t max_seq) {
  return gqa_decode_attn_num_splits((int)batch, (int)num_kv_heads,
                                    (int)max_seq);
}

// Decode linear: y[M,N] = x[M,K] @ w[N,K]^T on the weight-streaming
// MFMA kernel (csrc/skinny_gemm.hip). Caller guarantees M <= 64 and
// K % 128 == 0; larger M belongs to hipBLASLt. With w_scale the weights are
// weight-only fp8 (W8A16): w is [N, K] e4m3 with per-channel scales [N];
// activations stay bf16, dequantization happens in-fragment and the scale
// folds into the store (W_FP8).
torch::Tensor skinny_linear_impl(const torch::Tensor& x,
                                 const torch::Tensor& w,
                                 const c10::optional<torch::Tensor>& w_scale) {
  check_bf16_contig(x, "x");
  const float* scale_ptr = nullptr;
  if (w_scale.has_value()) {
    TORCH_CHECK(w.is_cuda() && w.is_contiguous() &&
                    w.scalar_type() == at::kFloat8_e4m3fn,
                "w must be contiguous float8_e4m3fn");
    TORCH_CHECK(w_scale->is_cuda() &&
                    w_scale->scalar_type() == torch::kFloat &&
                    w_scale->is_contiguous() && w.dim() == 2 &&
                    w_scale->numel() == w.size(0),
                "w_scale must be float32 [N]");
    scale_ptr = w_scale->data_ptr<float>();
  } else {
    check_bf16_contig(w, "w");
  }
  TORCH_CHECK(x.dim() == 2 && w.dim() == 2, "x [M,K], w [N,K]");
  const int M = x.size(0);
  const int K = x.size(1);
  const int N = w.size(0);
  TORCH_CHECK(w.size(1) == K, "K mismatch");
  TORCH_CHECK(M <= 64, "skinny_linear requires M <= 64");
  TORCH_CHECK(K % 128 == 0, "K must be a multiple of 128");
  auto y = torch::empty({M, N}, x.options());
  // N == 0 is a zero-sized GEMM grid and M == 0 a zero-sized merge grid:
  // both are invalid launches, and there is nothing to compute
  if (M == 0 || N == 0) return y;
  const int sk = skinny_gemm_num_splits(N, K, skinny_gemm_tile_n(M));
  torch::Tensor ws;
  void* ws_ptr = nullptr;
  if (sk > 1) {
    ws = torch::empty({(long)sk * M * N},
                      x.options().dtype(torch::kFloat32));
    ws_ptr = ws.data_ptr();
  }
  launch_skinny_gemm(y.data_ptr(), ws_ptr, x.data_ptr(), w.data_ptr(),
                     scale_ptr, M, N, K, sk, scale_ptr ? 1 : 0,
                     current_stream());
  return y;
}

torch::Tensor skinny_linear(torch::Tensor x, torch::Tensor w) {
  return skinny_linear_impl(x, w, c10::nullopt);
}

torch::Tensor skinny_linear_fp8(torch::Tensor x, torch::Tensor w,
                                torch::Tensor w_scale) {
  return skinny_linear_impl(x, w, w_scale);
}

// The split-K factor skinny_linear picks for x [M, K] and w [N, K] (the same
// for bf16 and fp8 weights); read-only, for tests that mean to exercise one.
int64_t skinny_linear_splits(int64_t M, int64_t N, int64_t K) {
  TORCH_CHECK(M >= 0 && M <= 64, "skinny_linear requires M <= 64");
  TORCH_CHECK(N >= 0 && N < (1L << 31), "N out of range");
  TORCH_CHECK(K >= 0 && K < (1L << 31) && K % 128 == 0,
              "K must be a multiple of 128");
  return skinny_gemm_num_splits((int)N, (int)K, skinny_gemm_tile_n((int)M));
}

// Operand checks shared by prefill_attn, extend_attn and extend_attn_ragged:
// q [T, Hq, 128] bf16 against head-major caches [>= batch, Hk, S_max, 128]
// with G = Hq / Hk <= 8.
struct PrefillOperands {
  bool kv_fp8;
  int num_q_heads, num_kv_heads, max_seq;
};

PrefillOperands check_prefill_operands(const torch::Tensor& q,
                                       const torch::Tensor& k_cache,
                                       const torch::Tensor& v_cache,
                                       int64_t batch) {
  check_bf16_contig(q, "q");
  const bool kv_fp8 = check_kv_pair(k_cache, v_cache);
  TORCH_CHECK(q.dim() == 3 && q.size(2) == 128, "q must be [T, Hq, 128]");
  TORCH_CHECK(k_cache.dim() == 4 && k_cache.size(3) == 128,
              "k_cache must be [B, Hk, S_max, 128]");
  TORCH_CHECK(k_cache.size(0) >= batch, "cache holds fewer than B sequences");
  const int num_q_heads = q.size(1);
  const int num_kv_heads = k_cache.size(1);
  TORCH_CHECK(num_q_heads % num_kv_heads == 0, "Hq must divide by Hk");
  TORCH_CHECK(num_q_heads / num_kv_heads <= 8, "GQA group size must be <= 8");
  return {kv_fp8, num_q_heads, num_kv_heads, (int)k_cache.size(2)};
}

// Causal flash-attention prefill over the (already-populated) head-major
// KV caches (csrc/prefill_attention.hip). q/out: [B*S, Hq, 128].
torch::Tensor prefill_attn(torch::Tensor q, torch::Tensor k_cache,
                           torch::Tensor v_cache, int64_t batch, int64_t seq,
                           double scale) {
  const PrefillOperands p = check_prefill_operands(q, k_cache, v_cache, batch);
  TORCH_CHECK(batch >= 0 && seq >= 0 && q.size(0) == batch * seq,
              "T must equal B*S");
  TORCH_CHECK(seq <= p.max_seq, "seq exceeds cache size");
  auto out = torch::empty_like(q);
  launch_prefill_attn(out.data_ptr(), q.data_ptr(), k_cache.data_ptr(),
                      v_cache.data_ptr(), nullptr, (int)batch, (int)seq,
                      p.num_q_heads, p.num_kv_heads, p.max_seq, (float)scale,
                      p.kv_fp8 ? 1 : 0, current_stream());
  return out;
}

// Chunked prefill ("extend") attention: `chunk` new query rows per sequence
// attend to a cached prefix of prefix_lens[b] rows plus the chunk's own
// rows, which the caller has already written at prefix_lens[b] ..
// prefix_lens[b]+chunk-1 (csrc/prefill_attention.hip, HAS_PREFIX).
// q/out: [B*chunk, Hq, 128]; prefix_lens stays on the device.
torch::Tensor extend_attn(torch::Tensor q, torch::Tensor k_cache,
                          torch::Tensor v_cache, torch::Tensor prefix_lens,
                          int64_t chunk, double scale) {
  check_i32_contig(prefix_lens, "prefix_lens");
  TORCH_CHECK(q.dim() == 3 && chunk >= 1 && q.size(0) % chunk == 0,
              "q must be [T, Hq, 128] with T a multiple of chunk");
  const int64_t batch = q.size(0) / chunk;
  const PrefillOperands p = check_prefill_operands(q, k_cache, v_cache, batch);
  TORCH_CHECK(prefix_lens.dim() == 1 && prefix_lens.size(0) == batch,
              "prefix_lens must be [B] with B = T / chunk");
  TORCH_CHECK(chunk <= p.max_seq, "chunk exceeds cache size");
  auto out = torch::empty_like(q);
  launch_prefill_attn(out.data_ptr(), q.data_ptr(), k_cache.data_ptr(),
                      v_cache.data_ptr(), prefix_lens.data_ptr<int>(),
                      (int)batch, (int)chunk, p.num_q_heads, p.num_kv_heads,
                      p.max_seq, (float)scale, p.kv_fp8 ? 1 : 0,
                      current_stream());
  return out;
}

// Ragged chunked prefill: sequence b owns the chunk_lens[b] <= max_chunk
// packed rows of q from q_starts[b] and continues from prefix_lens[b]; all
// three stay on the device (csrc/prefill_attention.hip, RAGGED). q/out:
// [T, Hq, 128]; rows that no sequence owns read as 0. num_splits > 1 splits
// the kv sweep over a workspace and merges (extend_attn_ragged_splits gives
// the launch heuristic's count).
torch::Tensor extend_attn_ragged(torch::Tensor q, torch::Tensor k_cache,
                                 torch::Tensor v_cache,
                                 torch::Tensor prefix_lens,
                                 torch::Tensor q_starts,
                                 torch::Tensor chunk_lens, int64_t max_chunk,
                                 double scale, int64_t num_splits) {
  check_i32_contig(prefix_lens, "prefix_lens");
  check_i32_contig(q_starts, "q_starts");
  check_i32_contig(chunk_lens, "chunk_lens");
  TORCH_CHECK(chunk_lens.dim() == 1 && chunk_lens.size(0) >= 1,
              "chunk_lens must be [B] with B >= 1");
  const int64_t batch = chunk_lens.size(0);
  const PrefillOperands p = check_prefill_operands(q, k_cache, v_cache, batch);
  const int num_q_heads = p.num_q_heads;
  TORCH_CHECK(q.size(0) >= 1, "need at least one query row");
  TORCH_CHECK(prefix_lens.dim() == 1 && prefix_lens.size(0) == batch,
              "prefix_lens must be [B] like chunk_lens");
  TORCH_CHECK(q_starts.dim() == 1 && q_starts.size(0) == batch,
              "q_starts must be [B] like chunk_lens");
  TORCH_CHECK(max_chunk >= 1 && max_chunk <= p.max_seq,
              "max_chunk must be in [1, cache size]");
  TORCH_CHECK(q.size(0) < (1L << 31) / num_q_heads, "T * Hq too large");
  const int64_t tiles = (max_chunk + 63) / 64;
  TORCH_CHECK(tiles <= 65535 && batch * num_q_heads < (1L << 31),
              "launch grid too large");
  TORCH_CHECK(num_splits >= 1 && num_splits <= 65535,
              "num_splits must be in [1, 65535]");
  auto out = torch::zeros_like(q);
  torch::Tensor ws;
  void* ws_ptr = nullptr;
  if (num_splits > 1) {
    const int64_t floats =
        batch * num_q_heads * tiles * 64 * num_splits * (2 + 128);
    TORCH_CHECK(floats <= (1L << 28),
                "split workspace would exceed 1 GiB; use fewer splits");
    ws = torch::empty({floats}, q.options().dtype(torch::kFloat32));
    ws_ptr = ws.data_ptr();
  }
  launch_extend_attn_ragged(
      out.data_ptr(), ws_ptr, q.data_ptr(), k_cache.data_ptr(),
      v_cache.data_ptr(), prefix_lens.data_ptr<int>(),
      q_starts.data_ptr<int>(), chunk_lens.data_ptr<int>(), (int)batch,
      (int)q.size(0), (int)max_chunk, num_q_heads, p.num_kv_heads, p.max_seq,
      (int)num_splits, (float)scale, p.kv_fp8 ? 1 : 0, current_stream());
  return out;
}

int64_t extend_attn_ragged_splits(int64_t batch, int64_t num_q_heads,
                                  int64_t max_chunk, int64_t max_seq) {
  return extend_attn_ragged_num_splits((int)batch, (int)num_q_heads,
                                       (int)max_chunk, (int)max_seq);
}

// --- routed MoE expert MLP (csrc/moe.hip) ---

// The m-tile grid dimension is launched at its static bound; keep it (and
// every int index the kernels form) comfortably in range.
void check_moe_sizes(long T, long E, long K) {
  TORCH_CHECK(T >= 1, "need at least one token");
  TORCH_CHECK(E >= 1 && E <= 64, "num_experts must be in [1, 64]");
  TORCH_CHECK(K >= 1 && K <= 8 && K <= E, "top_k must be in [1, min(8, E)]");
  TORCH_CHECK(T * K < (1L << 30), "T * top_k too large");
  TORCH_CHECK(moe_num_m_tiles((int)(T * K), (int)E) <= 65535,
              "too many m-tiles for one launch");
}

// router_logits fp32 [T, E] → (topk_idx [T,K] i32, topk_w [T,K] f32,
// expert_offsets [E+1] i32, sorted_slots [T*K] i32), all on device.
std::vector<torch::Tensor> moe_route(torch::Tensor router_logits,
                                     int64_t top_k) {
  TORCH_CHECK(router_logits.is_cuda(), "router_logits must be on GPU");
  TORCH_CHECK(router_logits.scalar_type() == torch::kFloat,
              "router_logits must be float32");
  TORCH_CHECK(router_logits.is_contiguous(),
              "router_logits must be contiguous");
  TORCH_CHECK(router_logits.dim() == 2, "router_logits must be [T, E]");
  const long T = router_logits.size(0);
  const long E = router_logits.size(1);
  check_moe_sizes(T, E, top_k);
  auto i32 = router_logits.options().dtype(torch::kInt32);
  auto topk_idx = torch::empty({T, top_k}, i32);
  auto topk_w = torch::empty({T, top_k}, router_logits.options());
  auto expert_offsets = torch::empty({E + 1}, i32);
  auto sorted_slots = torch::empty({T * top_k}, i32);
  launch_moe_route(topk_idx.data_ptr<int>(), topk_w.data_ptr<float>(),
                   expert_offsets.data_ptr<int>(),
                   sorted_slots.data_ptr<int>(),
                   router_logits.data_ptr<float>(), (int)T, (int)E,
                   (int)top_k, current_stream());
  return {topk_idx, topk_w, expert_offsets, sorted_slots};
}

// act_sorted [T*K, I] = silu(g)·u of x[token] · w_gate_up[e]^T, rows in
// expert-sorted order. w_gate_up is the stacked [E, 2I, H] tensor.
torch::Tensor moe_gate_up_swiglu(torch::Tensor x, torch::Tensor w_gate_up,
                                 torch::Tensor expert_offsets,
                                 torch::Tensor sorted_slots, int64_t top_k) {
  check_bf16_contig(x, "x");
  check_bf16_contig(w_gate_up, "w_gate_up");
  check_i32_contig(expert_offsets, "expert_offsets");
  check_i32_contig(sorted_slots, "sorted_slots");
  TORCH_CHECK(x.dim() == 2 && w_gate_up.dim() == 3,
              "x [T,H], w_gate_up [E,2I,H]");
  const long T = x.size(0);
  const long H = x.size(1);
  const long E = w_gate_up.size(0);
  check_moe_sizes(T, E, top_k);
  TORCH_CHECK(w_gate_up.size(2) == H, "H mismatch");
  TORCH_CHECK(w_gate_up.size(1) % 2 == 0, "w_gate_up rows must be 2*I");
  const long I = w_gate_up.size(1) / 2;
  TORCH_CHECK(H % 128 == 0, "H (K-dim) must be a multiple of 128");
  TORCH_CHECK(I % 16 == 0, "I (N-dim) must be a multiple of 16");
  TORCH_CHECK(expert_offsets.numel() == E + 1, "expert_offsets must be [E+1]");
  TORCH_CHECK(sorted_slots.numel() == T * top_k,
              "sorted_slots must be [T*top_k]");
  auto act = torch::empty({T * top_k, I}, x.options());
  launch_moe_gate_up_swiglu(act.data_ptr(), x.data_ptr(),
                            w_gate_up.data_ptr(),
                            expert_offsets.data_ptr<int>(),
                            sorted_slots.data_ptr<int>(), (int)T, (int)E,
                            (int)top_k, (int)H, (int)I, current_stream());
  return act;
}

// out [T, H] = Σ_k topk_w[t,k] · (act_sorted[pos(t,k)] · w_down[e]^T),
// w_down the stacked [E, H, I] tensor; split-K partials go through an
// fp32 workspace indexed by slot and are summed in a fixed order.
torch::Tensor moe_down_combine(torch::Tensor act_sorted, torch::Tensor w_down,
                               torch::Tensor topk_w,
                               torch::Tensor expert_offsets,
                               torch::Tensor sorted_slots) {
  check_bf16_contig(act_sorted, "act_sorted");
  check_bf16_contig(w_down, "w_down");
  check_i32_contig(expert_offsets, "expert_offsets");
  check_i32_contig(sorted_slots, "sorted_slots");
  TORCH_CHECK(topk_w.is_cuda() && topk_w.scalar_type() == torch::kFloat &&
                  topk_w.is_contiguous() && topk_w.dim() == 2,
              "topk_w must be contiguous float32 [T, K] on GPU");
  TORCH_CHECK(act_sorted.dim() == 2 && w_down.dim() == 3,
              "act_sorted [T*K,I], w_down [E,H,I]");
  const long T = topk_w.size(0);
  const long K = topk_w.size(1);
  const long E = w_down.size(0);
  const long H = w_down.size(1);
  const long I = w_down.size(2);
  check_moe_sizes(T, E, K);
  TORCH_CHECK(act_sorted.size(0) == T * K && act_sorted.size(1) == I,
              "act_sorted shape mismatch");
  TORCH_CHECK(I % 128 == 0, "I (K-dim) must be a multiple of 128");
  TORCH_CHECK(H % 16 == 0, "H (N-dim) must be a multiple of 16");
  TORCH_CHECK(expert_offsets.numel() == E + 1, "expert_offsets must be [E+1]");
  TORCH_CHECK(sorted_slots.numel() == T * K, "sorted_slots must be [T*K]");
  const int sk = moe_down_num_splits((int)(T * K), (int)E, (int)H, (int)I);
  auto ws = torch::empty({(long)sk * T * K * H},
                         act_sorted.options().dtype(torch::kFloat32));
  auto out = torch::empty({T, H}, act_sorted.options());
  launch_moe_down_combine(out.data_ptr(), ws.data_ptr<float>(),
                          act_sorted.data_ptr(), w_down.data_ptr(),
                          topk_w.data_ptr<float>(),
                          expert_offsets.data_ptr<int>(),
                          sorted_slots.data_ptr<int>(), (int)T, (int)E,
                          (int)K, (int)H, (int)I, sk, current_stream());
  return out;
}

int64_t moe_down_splits(int64_t tokens, int64_t top_k, int64_t num_experts,
                        int64_t hidden, int64_t inter) {
  return moe_down_num_splits((int)(tokens * top_k), (int)num_experts,
                             (int)hidden, (int)inter);
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("rmsnorm", &rmsnorm, "Fused (add-)RMSNorm bf16",
        py::arg("input"), py::arg("weight"), py::arg("residual") = py::none(),
        py::arg("eps") = 1e-5);
  m.def("rope", &rope, "Fused in-place NeoX RoPE on q,k",
        py::arg("q"), py::arg("k"), py::arg("positions"),
        py::arg("theta") = 500000.0);
  m.def("silu_mul", &silu_mul, "Fused SwiGLU silu(gate)*up",
        py::arg("gate"), py::arg("up"));
  m.def("silu_mul_fused", &silu_mul_fused,
        "SwiGLU on the fused [rows, 2*inter] gate_up buffer",
        py::arg("gate_up"));
  m.def("rope_append_kv", &rope_append_kv,
        "RoPE on strided qkv row + KV-cache append; returns contiguous q",
        py::arg("qkv"), py::arg("k_cache"), py::arg("v_cache"),
        py::arg("positions"), py::arg("num_q_heads"), py::arg("num_kv_heads"),
        py::arg("theta") = 500000.0);
  m.def("gqa_decode_attn", &gqa_decode_attn,
        "GQA decode attention over contiguous KV cache; variant pins the "
        "kernel (\"v4\", \"v5\") instead of the measured dispatch (\"auto\"), "
        "num_splits the split-KV factor instead of the launch heuristic",
        py::arg("q"), py::arg("k_cache"), py::arg("v_cache"),
        py::arg("context_lens"), py::arg("scale"),
        py::arg("variant") = "auto", py::arg("num_splits") = py::none());
  m.def("gqa_decode_attn_splits", &gqa_decode_attn_splits,
        "Split-KV factor gqa_decode_attn uses for a [batch, num_kv_heads, "
        "max_seq, 128] cache",
        py::arg("batch"), py::arg("num_kv_heads"), py::arg("max_seq"));
  m.def("rope_append_kv_paged", &rope_append_kv_paged,
        "RoPE on strided qkv row + append into a paged KV pool through "
        "block tables; returns contiguous q",
        py::arg("qkv"), py::arg("k_pages"), py::arg("v_pages"),
        py::arg("block_tables"), py::arg("positions"), py::arg("num_q_heads"),
        py::arg("num_kv_heads"), py::arg("theta") = 500000.0);
  m.def("paged_decode_attn", &paged_decode_attn,
        "GQA decode attention over a paged KV pool [num_blocks, Hk, "
        "block_size, 128] through block tables [B, max_blocks]",
        py::arg("q"), py::arg("k_pages"), py::arg("v_pages"),
        py::arg("block_tables"), py::arg("context_lens"), py::arg("scale"),
        py::arg("num_splits") = py::none(), py::arg("variant") = "auto");
  m.def("prefill_attn", &prefill_attn,
        "Causal flash-attention prefill over head-major KV caches",
        py::arg("q"), py::arg("k_cache"), py::arg("v_cache"),
        py::arg("batch"), py::arg("seq"), py::arg("scale"));
  m.def("extend_attn", &extend_attn,
        "Chunked-prefill attention: a chunk of query rows per sequence over "
        "a cached prefix (device-side prefix_lens)",
        py::arg("q"), py::arg("k_cache"), py::arg("v_cache"),
        py::arg("prefix_lens"), py::arg("chunk"), py::arg("scale"));
  m.def("extend_attn_ragged", &extend_attn_ragged,
        "Ragged chunked-prefill attention: chunk_lens[b] packed query rows "
        "per sequence from q_starts[b] over a cached prefix, optional "
        "split-KV (all per-sequence tensors on the device)",
        py::arg("q"), py::arg("k_cache"), py::arg("v_cache"),
        py::arg("prefix_lens"), py::arg("q_starts"), py::arg("chunk_lens"),
        py::arg("max_chunk"), py::arg("scale"), py::arg("num_splits"));
  m.def("extend_attn_ragged_splits", &extend_attn_ragged_splits,
        "Split-KV factor extend_attn_ragged picks for these static shapes",
        py::arg("batch"), py::arg("num_q_heads"), py::arg("max_chunk"),
        py::arg("max_seq"));
  m.def("skinny_linear_fp8", &skinny_linear_fp8,
        "Weight-only fp8 decode GEMM: x[M,K]bf16 @ w[N,K]e4m3^T, M <= 64",
        py::arg("x"), py::arg("w"), py::arg("w_scale"));
  m.def("skinny_linear", &skinny_linear,
        "Weight-streaming decode GEMM: x[M,K] @ w[N,K]^T, M <= 64",
        py::arg("x"), py::arg("w"));
  m.def("skinny_linear_splits", &skinny_linear_splits,
        "Split-K factor skinny_linear picks for x [M, K] and w [N, K]",
        py::arg("M"), py::arg("N"), py::arg("K"));
  m.def("moe_route", &moe_route,
        "MoE routing: top-k, softmax weights, expert offsets, sorted slots",
        py::arg("router_logits"), py::arg("top_k"));
  m.def("moe_gate_up_swiglu", &moe_gate_up_swiglu,
        "Grouped gate_up GEMM + SwiGLU over expert-sorted rows",
        py::arg("x"), py::arg("w_gate_up"), py::arg("expert_offsets"),
        py::arg("sorted_slots"), py::arg("top_k"));
  m.def("moe_down_combine", &moe_down_combine,
        "Grouped down GEMM + deterministic top-k combine",
        py::arg("act_sorted"), py::arg("w_down"), py::arg("topk_w"),
        py::arg("expert_offsets"), py::arg("sorted_slots"));
  m.def("moe_down_splits", &moe_down_splits,
        "Split-K factor moe_down_combine uses for these static shapes",
        py::arg("tokens"), py::arg("top_k"), py::arg("num_experts"),
        py::arg("hidden"), py::arg("inter"));
}
