// Fused rotary position embedding (NeoX/Llama style, non-interleaved
// half-rotation) — MI355X (gfx950).
//
// Two entry points:
//  * rope_kernel: in-place RoPE on contiguous q [T,Hq,D] / k [T,Hk,D]
//    (kept for tests and generic use).
//  * rope_append_kv_kernel: the decode fast path. Reads the UN-SLICED
//    qkv GEMM output row [B, (Hq+2Hk)·D] directly (no .contiguous()
//    copies), applies RoPE to q and k, writes q to a contiguous output
//    and APPENDS rotated k and raw v into the KV cache at each sequence's
//    current position — replacing 2 slice-copies + rope + 2 cache
//    index-writes per layer with one launch
//    (profiles/: ~13% of decode step time was this glue). The PAGED
//    instantiations append into a paged pool [num_blocks, Hk, block_size,
//    D] through block tables; the rotation code is the same.
//
// Grid: one workgroup per token; 256 threads cover heads × D/2 pairs.

#include "common.h"
#include "launch.h"

// bf16 destinations: float32 inv_freq and angle, hardware sin/cos (which
// reduces its argument itself). Measured against a float64 rotation this
// stays within one bf16 rounding plus half the float32-angle allowance of
// tests/attn_oracle.py up to position 131071.
__device__ __forceinline__ void rotate_pair(
    const bf16* src, bf16* dst, int d, int half, int head_dim, float pos,
    float theta) {
  const float inv_freq = __powf(theta, -2.0f * (float)d / (float)head_dim);
  const float angle = pos * inv_freq;
  float c, s;
  __sincosf(angle, &s, &c);
  const float x1 = bf2f(src[d]);
  const float x2 = bf2f(src[d + half]);
  dst[d] = f2bf(x1 * c - x2 * s);
  dst[d + half] = f2bf(x2 * c + x1 * s);
}

// fp8 cache only: cos and sin of pos · theta^(-2d/head_dim) from a double
// angle. At 128k positions the angle reaches 1.3e5 rad, where float32 is
// spaced 2^-7 rad apart and a float32 inv_freq is off by as much again.
// e4m3 steps are absolute (2^-9) below 2^-6, so a rotated K element near
// zero landed up to 3 steps from the exact rotation at position 131071 (1
// step from 8191 on). So inv_freq and the angle are formed in double,
// reduced there to a fraction of a turn, and the hardware sin/cos (whose
// argument is in turns) gets that fraction. A thread's pairs share d
// whenever blockDim.x is a multiple of head_dim/2, so the kernel keeps the
// last (d, cos, sin).
struct RopeCosSin {
  float c;
  float s;
};

__device__ __forceinline__ RopeCosSin rope_cos_sin(int d, int head_dim,
                                                   int pos,
                                                   double log2_theta) {
  const double inv_freq =
      exp2(-2.0 * (double)d / (double)head_dim * log2_theta);
  double turns = (double)pos * inv_freq * 0.15915494309189535;  // 1/(2π)
  turns -= floor(turns);
  const float t = (float)turns;
  return {__builtin_amdgcn_cosf(t), __builtin_amdgcn_sinf(t)};
}

// Last (d, cos, sin) a thread computed for its token.
struct RopeCosSinCache {
  int d = -1;
  RopeCosSin cs = {1.0f, 0.0f};

  __device__ __forceinline__ RopeCosSin get(int d_new, int head_dim, int pos,
                                            double log2_theta) {
    if (d_new != d) {
      cs = rope_cos_sin(d_new, head_dim, pos, log2_theta);
      d = d_new;
    }
    return cs;
  }
};

__device__ __forceinline__ void rotate_pair_cs(
    const bf16* src, bf16* dst, int d, int half, RopeCosSin cs) {
  const float x1 = bf2f(src[d]);
  const float x2 = bf2f(src[d + half]);
  dst[d] = f2bf(x1 * cs.c - x2 * cs.s);
  dst[d + half] = f2bf(x2 * cs.c + x1 * cs.s);
}

// Paged append target (PAGED instantiations): sequence b's row at position
// `pos` lives in page block_tables[b, pos / block_size], row pos %
// block_size, of a pool [num_blocks, Hk, block_size, D]. Returns the element
// offset of kv-head 0's row, or -1 when the row has no page: pos < 0,
// pos / block_size >= max_blocks (the table is not read then) or a table
// entry outside [0, num_blocks). The caller then skips the K/V stores, so a
// corrupt table or a position past the reservation never stores out of the
// pool; q_out is still produced.
__device__ __forceinline__ long paged_row_offset(
    const int* __restrict__ block_tables, int b, int pos, int max_blocks,
    int block_shift, int num_blocks, int num_kv_heads, int head_dim) {
  const int entry = pos >> block_shift;
  if (pos < 0 || entry >= max_blocks) return -1;
  const int id = block_tables[(long)b * max_blocks + entry];
  if (id < 0 || id >= num_blocks) return -1;
  const long row = (((long)id * num_kv_heads) << block_shift) +
                   (pos & ((1 << block_shift) - 1));
  return row * head_dim;
}

__global__ void rope_kernel(
    bf16* __restrict__ q,        // [T, Hq * D]
    bf16* __restrict__ k,        // [T, Hk * D]
    const int* __restrict__ positions,  // [T]
    const int num_q_heads,
    const int num_k_heads,
    const int head_dim,
    const float theta) {
  const int token = blockIdx.x;
  const float pos = (float)positions[token];
  const int half = head_dim / 2;
  const int total = (num_q_heads + num_k_heads) * half;

  for (int idx = threadIdx.x; idx < total; idx += blockDim.x) {
    const int head = idx / half;
    const int d = idx % half;
    const bool is_q = head < num_q_heads;
    bf16* base = is_q
        ? q + (long)token * num_q_heads * head_dim + (long)head * head_dim
        : k + (long)token * num_k_heads * head_dim +
              (long)(head - num_q_heads) * head_dim;
    rotate_pair(base, base, d, half, head_dim, pos, theta);
  }
}

template <bool PAGED>
__global__ void rope_append_kv_kernel(
    const bf16* __restrict__ qkv,   // [B, (Hq + 2·Hk) · D]
    bf16* __restrict__ q_out,       // [B, Hq, D]
    bf16* __restrict__ k_cache,     // [B, Hk, S_max, D] (head-major);
    bf16* __restrict__ v_cache,     // PAGED: [num_blocks, Hk, block_size, D]
    const int* __restrict__ positions,  // [B] append position per sequence
    const int num_q_heads,
    const int num_kv_heads,
    const int head_dim,
    const int max_seq,              // contiguous only
    const float theta,
    // PAGED only (null / 0 otherwise)
    const int* __restrict__ block_tables,  // [B, max_blocks]
    const int max_blocks,
    const int block_shift,          // log2(block_size)
    const int num_blocks) {
  const int b = blockIdx.x;
  const int pos_i = positions[b];
  const float pos = (float)pos_i;
  const int half = head_dim / 2;
  const long qkv_row = (long)b * (num_q_heads + 2 * num_kv_heads) * head_dim;
  // element offset of kv-head 0's row and the stride between kv-heads
  const long row0 =
      PAGED ? paged_row_offset(block_tables, b, pos_i, max_blocks, block_shift,
                               num_blocks, num_kv_heads, head_dim)
            : ((long)b * num_kv_heads * max_seq + pos_i) * head_dim;
  const long head_stride =
      PAGED ? (long)head_dim << block_shift : (long)max_seq * head_dim;
  const bool has_row = !PAGED || row0 >= 0;

  // q heads + k heads: rotate; v heads: straight copy (by 2-elem pairs)
  const int rot_total = (num_q_heads + num_kv_heads) * half;
  for (int idx = threadIdx.x; idx < rot_total; idx += blockDim.x) {
    const int head = idx / half;
    const int d = idx % half;
    if (head < num_q_heads) {
      const bf16* src = qkv + qkv_row + (long)head * head_dim;
      bf16* dst = q_out + ((long)b * num_q_heads + head) * head_dim;
      rotate_pair(src, dst, d, half, head_dim, pos, theta);
    } else {
      const int kh = head - num_q_heads;
      const bf16* src = qkv + qkv_row + ((long)num_q_heads + kh) * head_dim;
      bf16* dst = k_cache + row0 + kh * head_stride;
      if (has_row) rotate_pair(src, dst, d, half, head_dim, pos, theta);
    }
  }
  // v copy: vectorized bf16x2
  const int v_total = num_kv_heads * half;
  const bf16x2* vsrc = reinterpret_cast<const bf16x2*>(
      qkv + qkv_row + (long)(num_q_heads + num_kv_heads) * head_dim);
  for (int idx = threadIdx.x; idx < v_total; idx += blockDim.x) {
    const int kh = idx / half;
    const int d2 = idx % half;
    bf16x2* dst =
        reinterpret_cast<bf16x2*>(v_cache + row0 + kh * head_stride);
    if (has_row) dst[d2] = vsrc[(long)kh * half + d2];
  }
}

// fp8 (e4m3) cache variant of the decode append: q stays bf16; rotated
// k and copied v are down-converted to 1-byte e4m3 on store (half the
// cache bytes, double the KV capacity; see common.h fp8 helpers).
template <bool PAGED>
__global__ void rope_append_kv_fp8_kernel(
    const bf16* __restrict__ qkv,   // [B, (Hq + 2·Hk) · D]
    bf16* __restrict__ q_out,       // [B, Hq, D]
    fp8_t* __restrict__ k_cache,    // [B, Hk, S_max, D] e4m3;
    fp8_t* __restrict__ v_cache,    // PAGED: [num_blocks, Hk, block_size, D]
    const int* __restrict__ positions,
    const int num_q_heads,
    const int num_kv_heads,
    const int head_dim,
    const int max_seq,
    const double log2_theta,
    const int* __restrict__ block_tables,  // PAGED only, as in the bf16 kernel
    const int max_blocks,
    const int block_shift,
    const int num_blocks) {
  const int b = blockIdx.x;
  const int pos_i = positions[b];
  const int half = head_dim / 2;
  const long qkv_row = (long)b * (num_q_heads + 2 * num_kv_heads) * head_dim;
  const long row0 =
      PAGED ? paged_row_offset(block_tables, b, pos_i, max_blocks, block_shift,
                               num_blocks, num_kv_heads, head_dim)
            : ((long)b * num_kv_heads * max_seq + pos_i) * head_dim;
  const long head_stride =
      PAGED ? (long)head_dim << block_shift : (long)max_seq * head_dim;
  const bool has_row = !PAGED || row0 >= 0;

  const int rot_total = (num_q_heads + num_kv_heads) * half;
  RopeCosSinCache cache;
  for (int idx = threadIdx.x; idx < rot_total; idx += blockDim.x) {
    const int head = idx / half;
    const int d = idx % half;
    const RopeCosSin cs = cache.get(d, head_dim, pos_i, log2_theta);
    if (head < num_q_heads) {
      const bf16* src = qkv + qkv_row + (long)head * head_dim;
      bf16* dst = q_out + ((long)b * num_q_heads + head) * head_dim;
      rotate_pair_cs(src, dst, d, half, cs);
    } else {
      const int kh = head - num_q_heads;
      const bf16* src = qkv + qkv_row + ((long)num_q_heads + kh) * head_dim;
      const float x1 = bf2f(src[d]);
      const float x2 = bf2f(src[d + half]);
      fp8_t* dst = k_cache + row0 + kh * head_stride;
      if (has_row) {
        dst[d] = f2fp8(x1 * cs.c - x2 * cs.s);
        dst[d + half] = f2fp8(x2 * cs.c + x1 * cs.s);
      }
    }
  }
  // v copy: bf16x2 -> packed 2×e4m3 (adjacent dims), u16 stores
  const int v_total = num_kv_heads * half;
  const bf16x2* vsrc = reinterpret_cast<const bf16x2*>(
      qkv + qkv_row + (long)(num_q_heads + num_kv_heads) * head_dim);
  for (int idx = threadIdx.x; idx < v_total; idx += blockDim.x) {
    const int kh = idx / half;
    const int d2 = idx % half;
    const bf16x2 v2 = vsrc[(long)kh * half + d2];
    unsigned short* dst =
        reinterpret_cast<unsigned short*>(v_cache + row0 + kh * head_stride);
    if (has_row) dst[d2] = pk2_fp8(bf2f(v2.x), bf2f(v2.y));
  }
}

extern "C" void launch_rope(
    void* q, void* k, const int* positions, int tokens, int num_q_heads,
    int num_k_heads, int head_dim, float theta, hipStream_t stream) {
  dim3 grid(tokens);
  dim3 block(256);
  hipLaunchKernelGGL(rope_kernel, grid, block, 0, stream, (bf16*)q, (bf16*)k,
                     positions, num_q_heads, num_k_heads, head_dim, theta);
}

// The bf16 / e4m3 instantiation of one layout; the fp8 kernel takes
// log2(theta) as a double.
template <bool PAGED>
static void launch_append_kernel(
    const void* qkv, void* q_out, void* k_cache, void* v_cache,
    const int* positions, const PagedKV& p, int batch, int num_q_heads,
    int num_kv_heads, int head_dim, int max_seq, float theta, int kv_fp8,
    hipStream_t stream) {
  dim3 grid(batch);
  dim3 block(256);
  if (kv_fp8) {
    hipLaunchKernelGGL(rope_append_kv_fp8_kernel<PAGED>, grid, block, 0,
                       stream, (const bf16*)qkv, (bf16*)q_out, (fp8_t*)k_cache,
                       (fp8_t*)v_cache, positions, num_q_heads, num_kv_heads,
                       head_dim, max_seq, log2((double)theta), p.block_tables,
                       p.max_blocks, p.block_shift, p.num_blocks);
  } else {
    hipLaunchKernelGGL(rope_append_kv_kernel<PAGED>, grid, block, 0, stream,
                       (const bf16*)qkv, (bf16*)q_out, (bf16*)k_cache,
                       (bf16*)v_cache, positions, num_q_heads, num_kv_heads,
                       head_dim, max_seq, theta, p.block_tables, p.max_blocks,
                       p.block_shift, p.num_blocks);
  }
}

// The paged kernels take no max_seq (0), the contiguous ones no table.
extern "C" void launch_rope_append_kv(
    const void* qkv, void* q_out, void* k_cache, void* v_cache,
    const int* positions, const PagedKV* paged, int batch, int num_q_heads,
    int num_kv_heads, int head_dim, int max_seq, float theta, int kv_fp8,
    hipStream_t stream) {
  if (!paged) {
    launch_append_kernel<false>(qkv, q_out, k_cache, v_cache, positions,
                                PagedKV{nullptr, 0, 0, 0}, batch, num_q_heads,
                                num_kv_heads, head_dim, max_seq, theta, kv_fp8,
                                stream);
  } else {
    launch_append_kernel<true>(qkv, q_out, k_cache, v_cache, positions,
                               *paged, batch, num_q_heads, num_kv_heads,
                               head_dim, 0, theta, kv_fp8, stream);
  }
}
