// Host launch interface of the wva_amd MI355X (gfx950) kernels.
//
// Every host entry point of the .hip files is declared here, once. ops.cpp
// and each .hip file include this header, so a definition whose parameter
// list disagrees with its declaration is a compile error ("conflicting
// types") instead of a silent mismatch across C linkage. All tensor
// operands are device pointers; bf16 unless a comment says otherwise.
#pragma once

#include <hip/hip_runtime.h>

// Optional paged-pool operand of the decode attention and KV append
// launches. A null `const PagedKV*` selects the contiguous head-major cache
// [B, Hk, max_seq, D]; otherwise k/v are pools [num_blocks, Hk, block_size,
// D] with block_size = 1 << block_shift in {16, 32, 64}, addressed through
// block_tables, and the launch's max_seq argument is ignored.
struct PagedKV {
  const int* block_tables;  // [batch, max_blocks], device
  int max_blocks;
  int block_shift;          // log2(block_size)
  int num_blocks;
};

extern "C" {

// --- rmsnorm.hip ---
// out = rmsnorm(input [+ residual]) * weight over [rows, hidden], hidden %
// 8 == 0. residual may be null; otherwise residual_out receives input +
// residual (it may alias residual).
void launch_rmsnorm(void* out, void* residual_out, const void* input,
                    const void* residual, const void* weight, float eps,
                    int rows, int hidden, hipStream_t stream);

// --- rope.hip ---
// In-place NeoX RoPE on q [tokens, Hq, D] and k [tokens, Hk, D] at
// positions [tokens].
void launch_rope(void* q, void* k, const int* positions, int tokens,
                 int num_q_heads, int num_k_heads, int head_dim, float theta,
                 hipStream_t stream);
// Decode append: qkv [batch, (Hq + 2·Hk)·D] → RoPE'd q_out [batch, Hq, D],
// rotated k and raw v stored at positions[b] of the cache (bf16, or e4m3
// when kv_fp8). Contiguous caches are [batch, Hk, max_seq, D]; see PagedKV.
void launch_rope_append_kv(const void* qkv, void* q_out, void* k_cache,
                           void* v_cache, const int* positions,
                           const PagedKV* paged, int batch, int num_q_heads,
                           int num_kv_heads, int head_dim, int max_seq,
                           float theta, int kv_fp8, hipStream_t stream);

// --- silu_mul.hip ---
// out = silu(gate) * up over n elements, n even.
void launch_silu_mul(void* out, const void* gate, const void* up, long n,
                     hipStream_t stream);
// The same on the fused gate_up [rows, 2·inter] buffer; out [rows, inter].
void launch_silu_mul_fused(void* out, const void* gate_up, long rows,
                           long inter, hipStream_t stream);

// --- attention.hip ---
// Split-KV factor for a [batch, num_kv_heads, max_ctx_hint, 128] cache.
int gqa_decode_attn_num_splits(int batch, int num_kv_heads, int max_ctx_hint);
// Launch the chosen kernel (variant 4 or 5, bf16 or e4m3 cache, contiguous
// or paged) on a (batch, num_kv_heads, num_splits) grid, then the merge when
// the context was split. q/out [batch, Hq, 128], context_lens [batch].
// `workspace` holds batch·num_q_heads·num_splits·(2+128) floats; it may be
// null when num_splits == 1. Paged: the kernels see max_blocks · block_size
// as max_seq.
void launch_gqa_decode_attn(void* out, void* workspace, const void* q,
                            const void* k_cache, const void* v_cache,
                            const int* context_lens, const PagedKV* paged,
                            int batch, int num_q_heads, int num_kv_heads,
                            int max_seq, int num_splits, float scale,
                            int variant, int kv_fp8, hipStream_t stream);

// --- prefill_attention.hip ---
// Causal flash prefill of `rows` query rows per sequence over head-major
// caches [>= batch, Hk, max_seq, 128] (bf16 or e4m3); q/out [batch·rows, Hq,
// 128]; grid = (batch·Hq, ceil(rows/64)). prefix_lens [batch] gives the
// device-side offset of each sequence's chunk (chunked prefill); null means
// one-shot prefill from position 0.
void launch_prefill_attn(void* out, const void* q, const void* k_cache,
                         const void* v_cache, const int* prefix_lens,
                         int batch, int rows, int num_q_heads,
                         int num_kv_heads, int max_seq, float scale,
                         int kv_fp8, hipStream_t stream);
// Split count of the ragged extend launch, from static shapes only.
int extend_attn_ragged_num_splits(int batch, int num_q_heads, int max_chunk,
                                  int max_seq);
// Ragged chunked prefill: sequence b owns chunk_lens[b] <= max_chunk packed
// rows of q/out [total_rows, Hq, 128] from q_starts[b]; grid = (batch·Hq,
// ceil(max_chunk/64), num_splits), then the merge when the sweep was split.
// `ws` holds batch·Hq·ceil(max_chunk/64)·64·num_splits·(2+128) floats and may
// be null when num_splits == 1. Nothing is read back: graph-capturable.
void launch_extend_attn_ragged(void* out, void* ws, const void* q,
                               const void* k_cache, const void* v_cache,
                               const int* prefix_lens, const int* q_starts,
                               const int* chunk_lens, int batch,
                               int total_rows, int max_chunk, int num_q_heads,
                               int num_kv_heads, int max_seq, int num_splits,
                               float scale, int kv_fp8, hipStream_t stream);

// --- skinny_gemm.hip ---
// Workgroup N-tile width (64 or 128) for M rows, and the split-K factor for
// that width (power of two <= 16 dividing K/128).
int skinny_gemm_tile_n(int M);
int skinny_gemm_num_splits(int N, int K, int nt);
// c [M, N] = a [M, K] · w [N, K]^T, M <= 64, K % 128 == 0. w is bf16, or
// e4m3 with per-channel float scales w_scale [N] when w_fp8 (w_scale is
// null otherwise). `ws` holds num_splits·M·N floats and may be null when
// num_splits == 1.
void launch_skinny_gemm(void* c, void* ws, const void* a, const void* w,
                        const float* w_scale, int M, int N, int K,
                        int num_splits, int w_fp8, hipStream_t stream);

// --- moe.hip ---
// Static bound on non-empty m-tiles, n-subtiles per wave of the down GEMM,
// and its split-K factor (TK = tokens · top_k).
int moe_num_m_tiles(int TK, int E);
int moe_down_nsub(int TK);
int moe_down_num_splits(int TK, int E, int H, int I);
// logits float [T, E] → topk_idx [T, K], topk_w float [T, K],
// expert_offsets [E+1], sorted_slots [T·K].
void launch_moe_route(int* topk_idx, float* topk_w, int* expert_offsets,
                      int* sorted_slots, const float* logits, int T, int E,
                      int K, hipStream_t stream);
// act [T·top_k, I] = silu(g)·u of x [T, H] · w [E, 2I, H]^T, rows in
// expert-sorted order.
void launch_moe_gate_up_swiglu(void* act, const void* x, const void* w,
                               const int* expert_offsets,
                               const int* sorted_slots, int T, int E,
                               int top_k, int H, int I, hipStream_t stream);
// out [T, H] = Σ_k topk_w · (act · w [E, H, I]^T); `ws` holds
// num_splits·T·top_k·H floats and is always used.
void launch_moe_down_combine(void* out, float* ws, const void* act,
                             const void* w, const float* topk_w,
                             const int* expert_offsets,
                             const int* sorted_slots, int T, int E, int top_k,
                             int H, int I, int num_splits,
                             hipStream_t stream);

}  // extern "C"
