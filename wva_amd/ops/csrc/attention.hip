// GQA decode attention (single query token per sequence) over a
// contiguous head-major KV cache — MI355X (gfx950).
//
// Shape contract (Llama-3 family): head_dim = 128, G = Hq/Hk ≤ 8 query
// heads share one KV head; caches [B, Hk, S_max, 128] in bf16 or fp8
// e4m3 (KV_FP8 template). One 4-wave workgroup per (batch, kv_head,
// split).
//
// Two kernels (measured dispatch in ops.cpp), built from shared phases:
//   v4  MFMA scores: K streams HBM→VGPR fragments (no K staging), V via
//       LDS, VALU PV — best for G < 8 with split-KV
//   v5  v4 + MFMA PV (P cast to bf16, corr/s broadcast via LDS) — best
//       for G = 8 or unsplit grids
// plus the split-KV merge kernel. Both kernels also run over a paged pool
// [num_blocks, Hk, block_size, 128] addressed through block tables (PAGED
// template parameter): only the K row address, the staged V row's source
// and the clamp for positions past the context differ, see "Paged pool
// addressing" below. The Q-fragment build, the online-softmax
// step and the workspace addressing exist once, as __device__ helpers used
// by both kernels. V staging and the MFMA score tile are written out in
// each kernel: as helpers they compiled to different fp8 code that
// measured 1-2 % slower in v5. The optimization ladder with per-step
// measurements, the negative results along the way and the retired
// pre-MFMA v3 kernel are in docs/mi355x-kernels.md; MFMA
// fragment conventions were probe-verified on hardware
// (scripts/mfma_probe.hip): identical lane→k bijections for A and B
// suffice (the k-sum is permutation-invariant), C/D is col = lane&15,
// row = (lane>>4)·4 + reg.
//
// Host side: one entry, launch_gqa_decode_attn (declared in launch.h), picks
// the instantiation for both layouts and launches the merge.
#include "common.h"
#include "launch.h"

#include <type_traits>

#define HEAD_DIM 128
#define MAX_G 8
#define TILE 64            // positions per tile (= wave width)
#define NUM_WAVES 4
// LDS row stride in dwords: 66 = 64 + 2 pad. Even stride keeps every
// 8-byte access provably aligned (ds_read/write_b64) and banking stays
// conflict-free: b64 groups see banks (2·row + 2·d) mod 64 — distinct
// per lane; b32 PV reads see (2·t + lane) mod 32 — distinct per lane.
// (A 65-dword pad is conflict-free too but leaves every odd row 4-byte
// aligned, so the compiler silently splits vector LDS accesses.)
#define ROW_DW 66
#define S_ROW 65  // s_smem row stride (floats): 64 + 1 pad

// Cache element type of an instantiation.
template <bool KV_FP8>
using kv_elem_t = std::conditional_t<KV_FP8, fp8_t, bf16>;

// Split-KV: when the (B × Hk) grid is too small to fill 256 CUs (small
// batch / TP-8 70B decode), the context is additionally partitioned across
// blockIdx.z splits; each split writes (m, s, acc[128]) partials to a
// workspace [B, Hk, G, splits, 2 + 128] and the merge kernel combines
// them. splits == 1 takes the direct-store fast path. This is the float
// offset of one (b, kvh, g, split) row of that workspace.
__device__ __forceinline__ long ws_row_offset(int b, int kvh, int g, int split,
                                              int num_kv_heads, int G,
                                              int num_splits) {
  return ((((long)b * num_kv_heads + kvh) * G + g) * num_splits + split) *
         (2 + HEAD_DIM);
}

// Pack 8 floats (scaled into e4m3 range) into the fp8 MFMA operand.
__device__ __forceinline__ long pack8_fp8(const float* v, float inv_scale) {
  unsigned int lo = 0, hi = 0;
  lo = __builtin_amdgcn_cvt_pk_fp8_f32(v[0] * inv_scale, v[1] * inv_scale,
                                       lo, false);
  lo = __builtin_amdgcn_cvt_pk_fp8_f32(v[2] * inv_scale, v[3] * inv_scale,
                                       lo, true);
  hi = __builtin_amdgcn_cvt_pk_fp8_f32(v[4] * inv_scale, v[5] * inv_scale,
                                       hi, false);
  hi = __builtin_amdgcn_cvt_pk_fp8_f32(v[6] * inv_scale, v[7] * inv_scale,
                                       hi, true);
  return (long)(((unsigned long)hi << 32) | lo);
}

// Persistent Q operand of the score MFMA: B fragments, col = head =
// lane%16, k = 32·kk + 8·(lane/16) + i; heads ≥ G are zero. In fp8-KV
// mode Q is quantized ONCE per workgroup to e4m3 (`scale` is folded into
// the softmax scale by the score tile) so scores run on the fp8 MFMA with K
// bytes fed RAW — no per-fragment up-conversion on the hot path. Only the
// operand of the instantiation's own MFMA is live.
struct QFrags {
  bf16x8_frag bf[4];
  long fp8[4];
  float scale;
};

// `g` = lane%16 and `k0` = 8·(lane/16) are this lane's operand column and
// the first k of its group of 8. The kernel computes them once and uses
// the same values for its score tile: recomputed in here, the optimizer
// sinks the copies into the g < G branch, they stop folding with the later
// uses and the kernel's address arithmetic changes (v5 then compiles to
// 95/80 VGPRs instead of 127/124; see docs/mi355x-kernels.md).
// `qmax_lds` (fp8 only, NUM_WAVES floats) carries the cross-wave amax.
// Every thread of the workgroup must call this: the fp8 path has two
// barriers.
template <bool KV_FP8>
__device__ __forceinline__ QFrags load_q_frags(const bf16* __restrict__ q,
                                               int b, int kvh, int G,
                                               int num_q_heads, int lane,
                                               int wave, int g, int k0,
                                               float* qmax_lds) {
  QFrags qf;
  qf.scale = 1.0f;
#pragma unroll
  for (int kk = 0; kk < 4; ++kk) qf.fp8[kk] = 0;
  float qv[4][8];
#pragma unroll
  for (int kk = 0; kk < 4; ++kk)
#pragma unroll
    for (int i = 0; i < 8; ++i) qv[kk][i] = 0.0f;
  if (g < G) {
    const bf16* qrow = q + ((long)b * num_q_heads + kvh * G + g) * HEAD_DIM;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      const short* src = reinterpret_cast<const short*>(qrow + 32 * kk + k0);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        qf.bf[kk][i] = src[i];
        const bf16 bv = *reinterpret_cast<const bf16*>(&src[i]);
        qv[kk][i] = bf2f(bv);
      }
    }
  } else {
#pragma unroll
    for (int kk = 0; kk < 4; ++kk)
#pragma unroll
      for (int i = 0; i < 8; ++i) qf.bf[kk][i] = 0;
  }
  if constexpr (KV_FP8) {
    float amax = 0.0f;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk)
#pragma unroll
      for (int i = 0; i < 8; ++i) amax = fmaxf(amax, fabsf(qv[kk][i]));
    amax = wave_reduce_max(amax);
    if (lane == 0) qmax_lds[wave] = amax;
    __syncthreads();
    float m0 = qmax_lds[0];
#pragma unroll
    for (int w2 = 1; w2 < NUM_WAVES; ++w2) m0 = fmaxf(m0, qmax_lds[w2]);
    qf.scale = fmaxf(m0 / 448.0f, 1e-12f);
    const float inv = 1.0f / qf.scale;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) qf.fp8[kk] = pack8_fp8(qv[kk], inv);
    __syncthreads();  // qmax_lds consumed before any reuse
  }
  return qf;
}

// One online-softmax step of a wave-owned head over a score tile row
// (lane ↔ position). Updates the running max `m` and sum `s`; returns
// this lane's probability `p` and the factor `corr` by which everything
// accumulated before this tile must be rescaled.
struct SoftmaxStep {
  float p;
  float corr;
};

__device__ __forceinline__ SoftmaxStep online_softmax_step(
    const float* __restrict__ s_row, int tn, int lane, float& m, float& s) {
  const bool live = lane < tn;
  const float score = live ? s_row[lane] : -INFINITY;
  const float tile_max = wave_reduce_max(score);
  const float m_new = fmaxf(m, tile_max);
  const float p = live ? __expf(score - m_new) : 0.0f;
  const float tile_sum = wave_reduce_sum(p);
  const float corr = (m == -INFINITY) ? 0.0f : __expf(m - m_new);
  s = s * corr + tile_sum;
  m = m_new;
  return {p, corr};
}

// ---------------------------------------------------------------------------
// Paged pool addressing (PAGED instantiations only). k_pages / v_pages are
// [num_blocks, Hk, block_size, 128] with block_size in {16, 32, 64}, the
// divisors of TILE that are multiples of 16: one (page, kv-head) is a
// contiguous run of block_size rows, and each aligned group of 16 positions
// (a wave's 16 score rows, a wave's staged V rows of one pass) lies inside
// one page. block_tables is [B, max_blocks] int32; entry i of row b is the
// physical page of sequence b's positions i·block_size .. (i+1)·block_size−1.
//
// Rules that keep every access inside the pool whatever the tables hold:
//   * the effective context is min(context_lens[b], max_blocks·block_size);
//   * a position at or past the context is clamped to ctx − 1 BEFORE the
//     table lookup, so table entries at index >= ceil(ctx / block_size) are
//     never dereferenced;
//   * a physical id read from the table is clamped into [0, num_blocks − 1]
//     before it forms an address.
// A corrupt table therefore yields wrong numbers, never an out-of-bounds
// access.
// ---------------------------------------------------------------------------

// Physical page ids of a tile's four 16-position groups, fetched once per
// tile through wave-uniform indices (scalar loads), never per element.
struct TilePages {
  int id[4];

  // `group` is wave-uniform; a select chain keeps id[] in registers (a
  // runtime-indexed array would go to scratch).
  __device__ __forceinline__ int pick(int group) const {
    return group == 0 ? id[0] : group == 1 ? id[1] : group == 2 ? id[2] : id[3];
  }
};

// `table_row` = block_tables + b·max_blocks; t0 < ctx, ctx >= 1 already the
// effective context. Group g covers positions t0 + 16g .. t0 + 16g + 15; a
// group that starts at or past ctx takes the page of position ctx − 1, which
// is where its clamped rows read.
__device__ __forceinline__ TilePages load_tile_pages(
    const int* __restrict__ table_row, int t0, int ctx, int block_shift,
    int num_blocks) {
  const int last_block = (ctx - 1) >> block_shift;  // last entry ever read
  TilePages pages;
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const int entry = min((t0 + 16 * g) >> block_shift, last_block);
    const int id = table_row[entry];
    pages.id[g] = min(max(id, 0), num_blocks - 1);  // never leaves the pool
  }
  return pages;
}

// Row of position `pos` (< ctx) in its page. `head0` points at this kv-head's
// rows of page 0, `page_stride` = Hk·block_size·128 elements; the page
// offset is formed in 64-bit.
template <typename T>
__device__ __forceinline__ const T* page_row(const T* head0,
                                             const TilePages& pages, int group,
                                             int pos, int block_mask,
                                             long page_stride) {
  return head0 + (long)pages.pick(group) * page_stride +
         (long)(pos & block_mask) * HEAD_DIM;
}

// ---------------------------------------------------------------------------
// v4: MFMA scores, VALU PV. Wave w owns the softmax state and the output
// of heads w and w+4 (lane ↔ output dword); only V goes through LDS (the
// position-major PV sweep needs the transpose LDS provides). 2 barriers
// per tile.
// ---------------------------------------------------------------------------
template <bool KV_FP8, bool PAGED>
__global__ __launch_bounds__(256, 2) void gqa_decode_attn_v4_kernel(
    bf16* __restrict__ out,            // [B, Hq, 128]
    float* __restrict__ workspace,     // [B, Hk, G, splits, 2+128] or null
    const bf16* __restrict__ q,        // [B, Hq, 128]
    const void* __restrict__ k_cache,  // [B, Hk, S_max, 128] bf16 or e4m3;
    const void* __restrict__ v_cache,  // PAGED: [num_blocks, Hk, bs, 128]
    const int* __restrict__ context_lens,  // [B]
    const int num_q_heads,
    const int num_kv_heads,
    const int max_seq,                 // PAGED: max_blocks · block_size
    const float scale,
    // PAGED only (null / 0 otherwise)
    const int* __restrict__ block_tables,  // [B, max_blocks]
    const int max_blocks,
    const int block_shift,             // log2(block_size)
    const int num_blocks) {
  const int b = blockIdx.x;
  const int kvh = blockIdx.y;
  const int split = blockIdx.z;
  const int num_splits = gridDim.z;
  const int G = num_q_heads / num_kv_heads;
  // PAGED: effective context, see "Paged pool addressing"
  const int ctx =
      PAGED ? min(context_lens[b], max_seq) : context_lens[b];

  const int lane = threadIdx.x & (WAVE_SIZE - 1);
  const int wave = threadIdx.x / WAVE_SIZE;
  // this lane's MFMA operand coordinates, see load_q_frags
  const int frag_col = lane % 16;
  const int frag_k0 = 8 * (lane / 16);

  __shared__ float s_smem[MAX_G][S_ROW];      // score tile [head][pos]
  __shared__ unsigned int v_smem[TILE * ROW_DW];
  __shared__ float p_smem[MAX_G][TILE];
  float* qmax_lds = nullptr;
  if constexpr (KV_FP8) {
    __shared__ float qmax_smem[NUM_WAVES];
    qmax_lds = qmax_smem;
  }

  const QFrags qf = load_q_frags<KV_FP8>(q, b, kvh, G, num_q_heads, lane,
                                         wave, frag_col, frag_k0, qmax_lds);

  // Per-wave running softmax state for its owned heads (g = wave + j*4).
  const int heads_mine = (G > wave) ? (G - wave + NUM_WAVES - 1) / NUM_WAVES : 0;
  float m[2], s[2], acc[2][2];  // at most 2 heads per wave (G ≤ 8)
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    m[j] = -INFINITY;
    s[j] = 0.0f;
    acc[j][0] = acc[j][1] = 0.0f;
  }

  // head-major cache: this (b, kvh)'s positions are contiguous. PAGED:
  // k_slab / v_slab are this kv-head's rows of page 0.
  const long slab_off =
      PAGED ? (long)kvh << (block_shift + 7)
            : ((long)b * num_kv_heads + kvh) * max_seq * HEAD_DIM;
  const long page_stride = (long)num_kv_heads << (block_shift + 7);
  const int block_mask = (1 << block_shift) - 1;
  const int* table_row = block_tables + (long)b * max_blocks;
  const auto* k_slab =
      reinterpret_cast<const kv_elem_t<KV_FP8>*>(k_cache) + slab_off;
  const auto* v_slab =
      reinterpret_cast<const kv_elem_t<KV_FP8>*>(v_cache) + slab_off;

  // Interleave tiles across splits: split s takes tiles s, s+S, s+2S, ...
  for (int t0 = split * TILE; t0 < ctx; t0 += num_splits * TILE) {
    const int tn = min(TILE, ctx - t0);
    TilePages pages;
    if constexpr (PAGED)
      pages = load_tile_pages(table_row, t0, ctx, block_shift, num_blocks);

    // --- stage V only; the fp8 path up-converts during staging so the
    // LDS layout and PV sweep are identical in both modes ---
    if constexpr (KV_FP8) {
      const int tile_g8 = tn * (HEAD_DIM / 8);
      const fp8_t* v_src = v_slab + (long)t0 * HEAD_DIM;
      for (int idx = wave * WAVE_SIZE + lane; idx < tile_g8;
           idx += NUM_WAVES * WAVE_SIZE) {
        const int row = idx >> 4;          // 16 groups of 8 per row
        const int d8 = (idx & 15) * 8;
        const fp8_t* v_row;
        if constexpr (PAGED)  // a wave's 4 rows of a pass share a page
          v_row = page_row(v_slab, pages,
                           __builtin_amdgcn_readfirstlane(row >> 4), t0 + row,
                           block_mask, page_stride);
        else
          v_row = v_src + (long)row * HEAD_DIM;
        const unsigned short* src =
            reinterpret_cast<const unsigned short*>(v_row + d8);
        unsigned int* dst = &v_smem[row * ROW_DW + d8 / 2];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float2_vt f = unpk2_fp8(src[j]);
          const bf16x2 packed{f2bf(f[0]), f2bf(f[1])};
          dst[j] = *reinterpret_cast<const unsigned int*>(&packed);
        }
      }
    } else {
      typedef __attribute__((ext_vector_type(2))) unsigned int uint2_t;
      const int tile_u2 = tn * (HEAD_DIM / 4);
      const unsigned int* v_src =
          reinterpret_cast<const unsigned int*>(v_slab + (long)t0 * HEAD_DIM);
      for (int idx = wave * WAVE_SIZE + lane; idx < tile_u2;
           idx += NUM_WAVES * WAVE_SIZE) {
        const int row = idx >> 5;
        const int d2 = (idx & 31) * 2;
        const unsigned int* src;
        if constexpr (PAGED)  // a wave's 2 rows of a pass share a page
          src = reinterpret_cast<const unsigned int*>(page_row(
                    v_slab, pages, __builtin_amdgcn_readfirstlane(row >> 4),
                    t0 + row, block_mask, page_stride)) + d2;
        else
          src = &v_src[idx * 2];
        const uint2_t val = *reinterpret_cast<const uint2_t*>(src);
        *reinterpret_cast<uint2_t*>(&v_smem[row * ROW_DW + d2]) = val;
      }
    }

    // --- MFMA scores: wave w owns tile positions 16w..16w+15 ---
    {
      const int prow = 16 * wave + (lane % 16);       // A row = position
      const int pos = t0 + prow;
      // clamped load. PAGED clamps to the context (not the cache size)
      // before the table lookup; the wave's 16 rows share a page.
      const int pos_lim = PAGED ? ctx : max_seq;
      const int pos_c = pos < pos_lim ? pos : pos_lim - 1;
      const kv_elem_t<KV_FP8>* k_row;
      if constexpr (PAGED)
        k_row = page_row(k_slab, pages, __builtin_amdgcn_readfirstlane(wave),
                         pos_c, block_mask, page_stride);
      else
        k_row = k_slab + (long)pos_c * HEAD_DIM;
      const int k0 = frag_k0;
      f32x4_frag sf = {0.f, 0.f, 0.f, 0.f};
      if constexpr (KV_FP8) {
        // fp8×fp8 MFMA: K bytes fed raw (8 per lane, one b64 load);
        // Q was pre-quantized with scale q_scale
        const long* ksrc = reinterpret_cast<const long*>(k_row);
        const int l0 = k0 / 8;  // which 8-byte group this lane reads
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
          const long a8 = ksrc[kk * 4 + l0];
          sf = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(
              a8, qf.fp8[kk], sf, 0, 0, 0);
        }
      } else {
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
          bf16x8_frag a_frag;
          const short* src =
              reinterpret_cast<const short*>(k_row) + 32 * kk + k0;
#pragma unroll
          for (int i = 0; i < 8; ++i) a_frag[i] = src[i];
          sf = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a_frag, qf.bf[kk],
                                                       sf, 0, 0, 0);
        }
      }
      // C/D: col = lane&15 (head), row = (lane>>4)·4 + i (position);
      // fp8 path folds the Q quantization scale back in here
      const float s_eff = KV_FP8 ? scale * qf.scale : scale;
      const int g = lane & 15;
      if (g < G) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int t = 16 * wave + (lane >> 4) * 4 + i;
          s_smem[g][t] = (t < tn) ? sf[i] * s_eff : -INFINITY;
        }
      }
    }
    __syncthreads();  // V + scores visible

    // --- softmax per owned head; rescale the register accumulators ---
    for (int j = 0; j < heads_mine; ++j) {
      const int g = wave + j * NUM_WAVES;
      const SoftmaxStep st = online_softmax_step(s_smem[g], tn, lane, m[j], s[j]);
      acc[j][0] *= st.corr;
      acc[j][1] *= st.corr;
      p_smem[g][lane] = st.p;  // lane ↔ position, in-bounds (TILE == 64)
    }
    // Waves read only their OWN heads' p rows; the barrier below orders
    // the NEXT tile's staging against this compute.

    // --- PV: lane ↔ output dword, sweep tile positions ---
    for (int j = 0; j < heads_mine; ++j) {
      const int g = wave + j * NUM_WAVES;
      const float* pg = p_smem[g];
      float a0 = acc[j][0], a1 = acc[j][1];
      for (int t = 0; t < tn; ++t) {
        const unsigned int vw = v_smem[t * ROW_DW + lane];
        const bf16x2 vv = *reinterpret_cast<const bf16x2*>(&vw);
        const float p = pg[t];  // broadcast
        a0 = fmaf(p, bf2f(vv.x), a0);
        a1 = fmaf(p, bf2f(vv.y), a1);
      }
      acc[j][0] = a0;
      acc[j][1] = a1;
    }
    __syncthreads();  // compute done before next tile overwrites LDS
  }

  // --- finalize: the owning wave writes its heads ---
  if (num_splits == 1) {
    for (int j = 0; j < heads_mine; ++j) {
      const int g = wave + j * NUM_WAVES;
      const float inv = s[j] > 0.0f ? 1.0f / s[j] : 0.0f;
      bf16x2* orow = reinterpret_cast<bf16x2*>(
          out + ((long)b * num_q_heads + kvh * G + g) * HEAD_DIM);
      orow[lane] = bf16x2{f2bf(acc[j][0] * inv), f2bf(acc[j][1] * inv)};
    }
  } else {
    for (int j = 0; j < heads_mine; ++j) {
      const int g = wave + j * NUM_WAVES;
      float* wsp = workspace +
          ws_row_offset(b, kvh, g, split, num_kv_heads, G, num_splits);
      if (lane == 0) {
        wsp[0] = m[j];
        wsp[1] = s[j];
      }
      wsp[2 + 2 * lane] = acc[j][0];
      wsp[2 + 2 * lane + 1] = acc[j][1];
    }
  }
}

// ---------------------------------------------------------------------------
// v5: v4 + MFMA PV. PMC counters showed v4 issue-bound on VALU (4.07 G
// VALU vs 30 M MFMA instructions — the vector PV sweep, 64 positions ×
// 2 fma × heads per wave per tile). v5 computes O += P·V on the matrix
// cores too:
//   * P [16 heads × 64 pos] (zero-padded heads) as A fragments from
//     p_smem, cast fp32→bf16 at fragment build (FA2-standard precision);
//   * V as B fragments straight from v_smem u16 reads (no conversion —
//     V is bf16 in LDS);
//   * wave w owns head_dim n-subtiles {w, w+4} → 2 persistent f32x4
//     accumulators; online-softmax rescale multiplies each accumulator
//     register by corr[head(reg)] from LDS before the tile's 4 MFMAs.
// Needs one extra barrier per tile (every wave now reads every head's
// p row; 3 per tile plus one before the epilogue) and LDS broadcast of
// corr/s; softmax state stays wave-owned.
// ---------------------------------------------------------------------------
template <bool KV_FP8, bool PAGED>
__global__ __launch_bounds__(256, 2) void gqa_decode_attn_v5_kernel(
    bf16* __restrict__ out,
    float* __restrict__ workspace,
    const bf16* __restrict__ q,
    const void* __restrict__ k_cache,  // bf16 or e4m3 (KV_FP8)
    const void* __restrict__ v_cache,
    const int* __restrict__ context_lens,
    const int num_q_heads,
    const int num_kv_heads,
    const int max_seq,
    const float scale,
    const int* __restrict__ block_tables,  // PAGED only, as in v4
    const int max_blocks,
    const int block_shift,
    const int num_blocks) {
  const int b = blockIdx.x;
  const int kvh = blockIdx.y;
  const int split = blockIdx.z;
  const int num_splits = gridDim.z;
  const int G = num_q_heads / num_kv_heads;
  // PAGED: effective context, see "Paged pool addressing"
  const int ctx =
      PAGED ? min(context_lens[b], max_seq) : context_lens[b];

  const int lane = threadIdx.x & (WAVE_SIZE - 1);
  const int wave = threadIdx.x / WAVE_SIZE;
  // this lane's MFMA operand coordinates, see load_q_frags
  const int frag_col = lane % 16;
  const int frag_k0 = 8 * (lane / 16);

  __shared__ float s_smem[MAX_G][S_ROW];
  __shared__ unsigned int v_smem[TILE * ROW_DW];
  __shared__ float p_smem[MAX_G][TILE];
  __shared__ float corr_smem[MAX_G];
  __shared__ float sum_smem[MAX_G];
  __shared__ float m_smem[MAX_G];
  float* qmax_lds = nullptr;
  if constexpr (KV_FP8) {
    __shared__ float qmax_smem[NUM_WAVES];
    qmax_lds = qmax_smem;
  }

  const QFrags qf = load_q_frags<KV_FP8>(q, b, kvh, G, num_q_heads, lane,
                                         wave, frag_col, frag_k0, qmax_lds);

  const int heads_mine = (G > wave) ? (G - wave + NUM_WAVES - 1) / NUM_WAVES : 0;
  float m[2], s[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    m[j] = -INFINITY;
    s[j] = 0.0f;
  }
  // PV accumulators: wave owns n-subtiles wave and wave+4 of head_dim;
  // lane holds (head = (lane>>4)*4 + reg, dim = 16*nsub + lane&15).
  f32x4_frag acc_pv[2] = {f32x4_frag{0.f, 0.f, 0.f, 0.f},
                          f32x4_frag{0.f, 0.f, 0.f, 0.f}};

  const long slab_off =
      PAGED ? (long)kvh << (block_shift + 7)
            : ((long)b * num_kv_heads + kvh) * max_seq * HEAD_DIM;
  const long page_stride = (long)num_kv_heads << (block_shift + 7);
  const int block_mask = (1 << block_shift) - 1;
  const int* table_row = block_tables + (long)b * max_blocks;
  const auto* k_slab =
      reinterpret_cast<const kv_elem_t<KV_FP8>*>(k_cache) + slab_off;
  const auto* v_slab =
      reinterpret_cast<const kv_elem_t<KV_FP8>*>(v_cache) + slab_off;

  for (int t0 = split * TILE; t0 < ctx; t0 += num_splits * TILE) {
    const int tn = min(TILE, ctx - t0);
    TilePages pages;
    if constexpr (PAGED)
      pages = load_tile_pages(table_row, t0, ctx, block_shift, num_blocks);

    // --- stage V only; the fp8 path up-converts during staging so the
    // LDS layout and PV sweep are identical in both modes ---
    if constexpr (KV_FP8) {
      const int tile_g8 = tn * (HEAD_DIM / 8);
      const fp8_t* v_src = v_slab + (long)t0 * HEAD_DIM;
      for (int idx = wave * WAVE_SIZE + lane; idx < tile_g8;
           idx += NUM_WAVES * WAVE_SIZE) {
        const int row = idx >> 4;          // 16 groups of 8 per row
        const int d8 = (idx & 15) * 8;
        const fp8_t* v_row;
        if constexpr (PAGED)  // a wave's 4 rows of a pass share a page
          v_row = page_row(v_slab, pages,
                           __builtin_amdgcn_readfirstlane(row >> 4), t0 + row,
                           block_mask, page_stride);
        else
          v_row = v_src + (long)row * HEAD_DIM;
        const unsigned short* src =
            reinterpret_cast<const unsigned short*>(v_row + d8);
        unsigned int* dst = &v_smem[row * ROW_DW + d8 / 2];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float2_vt f = unpk2_fp8(src[j]);
          const bf16x2 packed{f2bf(f[0]), f2bf(f[1])};
          dst[j] = *reinterpret_cast<const unsigned int*>(&packed);
        }
      }
    } else {
      typedef __attribute__((ext_vector_type(2))) unsigned int uint2_t;
      const int tile_u2 = tn * (HEAD_DIM / 4);
      const unsigned int* v_src =
          reinterpret_cast<const unsigned int*>(v_slab + (long)t0 * HEAD_DIM);
      for (int idx = wave * WAVE_SIZE + lane; idx < tile_u2;
           idx += NUM_WAVES * WAVE_SIZE) {
        const int row = idx >> 5;
        const int d2 = (idx & 31) * 2;
        const unsigned int* src;
        if constexpr (PAGED)  // a wave's 2 rows of a pass share a page
          src = reinterpret_cast<const unsigned int*>(page_row(
                    v_slab, pages, __builtin_amdgcn_readfirstlane(row >> 4),
                    t0 + row, block_mask, page_stride)) + d2;
        else
          src = &v_src[idx * 2];
        const uint2_t val = *reinterpret_cast<const uint2_t*>(src);
        *reinterpret_cast<uint2_t*>(&v_smem[row * ROW_DW + d2]) = val;
      }
    }

    // --- MFMA scores: wave w owns tile positions 16w..16w+15 ---
    {
      const int prow = 16 * wave + (lane % 16);       // A row = position
      const int pos = t0 + prow;
      // clamped load. PAGED clamps to the context (not the cache size)
      // before the table lookup; the wave's 16 rows share a page.
      const int pos_lim = PAGED ? ctx : max_seq;
      const int pos_c = pos < pos_lim ? pos : pos_lim - 1;
      const kv_elem_t<KV_FP8>* k_row;
      if constexpr (PAGED)
        k_row = page_row(k_slab, pages, __builtin_amdgcn_readfirstlane(wave),
                         pos_c, block_mask, page_stride);
      else
        k_row = k_slab + (long)pos_c * HEAD_DIM;
      const int k0 = frag_k0;
      f32x4_frag sf = {0.f, 0.f, 0.f, 0.f};
      if constexpr (KV_FP8) {
        // fp8×fp8 MFMA: K bytes fed raw (8 per lane, one b64 load);
        // Q was pre-quantized with scale q_scale
        const long* ksrc = reinterpret_cast<const long*>(k_row);
        const int l0 = k0 / 8;  // which 8-byte group this lane reads
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
          const long a8 = ksrc[kk * 4 + l0];
          sf = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(
              a8, qf.fp8[kk], sf, 0, 0, 0);
        }
      } else {
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
          bf16x8_frag a_frag;
          const short* src =
              reinterpret_cast<const short*>(k_row) + 32 * kk + k0;
#pragma unroll
          for (int i = 0; i < 8; ++i) a_frag[i] = src[i];
          sf = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a_frag, qf.bf[kk],
                                                       sf, 0, 0, 0);
        }
      }
      // C/D: col = lane&15 (head), row = (lane>>4)·4 + i (position);
      // fp8 path folds the Q quantization scale back in here
      const float s_eff = KV_FP8 ? scale * qf.scale : scale;
      const int g = lane & 15;
      if (g < G) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int t = 16 * wave + (lane >> 4) * 4 + i;
          s_smem[g][t] = (t < tn) ? sf[i] * s_eff : -INFINITY;
        }
      }
    }
    __syncthreads();  // V + scores visible

    // --- softmax per owned head; publish p and corr ---
    for (int j = 0; j < heads_mine; ++j) {
      const int g = wave + j * NUM_WAVES;
      const SoftmaxStep st = online_softmax_step(s_smem[g], tn, lane, m[j], s[j]);
      p_smem[g][lane] = st.p;
      if (lane == 0) corr_smem[g] = st.corr;
    }
    // dead heads (g >= G) keep corr undefined; PV zero-pads their rows
    __syncthreads();  // p + corr visible to all waves

    // --- MFMA PV: O[16 heads × dims] += P[16×64] · V[64×dims] ---
    {
      // A fragments (P): shared by this wave's two n-subtiles
      bf16x8_frag p_frag[2];
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        const int g = lane % 16;
        const int pos0 = 32 * kk + 8 * (lane / 16);
        if (g < G) {
#pragma unroll
          for (int i = 0; i < 8; ++i)
            p_frag[kk][i] = f2bf_bits(p_smem[g][pos0 + i]);
        } else {
#pragma unroll
          for (int i = 0; i < 8; ++i) p_frag[kk][i] = 0;
        }
      }
      const unsigned short* v_u16 =
          reinterpret_cast<const unsigned short*>(v_smem);
#pragma unroll
      for (int nsub = 0; nsub < 2; ++nsub) {
        const int dim = 16 * (wave + 4 * nsub) + (lane % 16);
        // rescale accumulator by corr[head(reg)]
        f32x4_frag d = acc_pv[nsub];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int h = (lane >> 4) * 4 + i;
          d[i] *= (h < G) ? corr_smem[h] : 0.0f;
        }
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
          bf16x8_frag v_frag;
          const int pos0 = 32 * kk + 8 * (lane / 16);
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            const int t = pos0 + i;
            // t >= tn rows are unstaged (stale LDS can decode to NaN,
            // and 0·NaN = NaN even though p[t] = 0) — zero them
            v_frag[i] = (t < tn)
                ? (short)v_u16[(t * ROW_DW + (dim >> 1)) * 2 + (dim & 1)]
                : (short)0;
          }
          d = __builtin_amdgcn_mfma_f32_16x16x32_bf16(p_frag[kk], v_frag, d,
                                                      0, 0, 0);
        }
        acc_pv[nsub] = d;
      }
    }
    __syncthreads();  // PV consumed V/p before next tile overwrites
  }

  // publish per-head softmax sums (and maxima for the split path)
  for (int j = 0; j < heads_mine; ++j) {
    const int g = wave + j * NUM_WAVES;
    if (lane == 0) {
      sum_smem[g] = s[j];
      m_smem[g] = m[j];
    }
  }
  __syncthreads();

  // lane holds (head = (lane>>4)*4+reg, dim = 16*(wave+4*nsub)+lane&15)
  if (num_splits == 1) {
#pragma unroll
    for (int nsub = 0; nsub < 2; ++nsub) {
      const int dim = 16 * (wave + 4 * nsub) + (lane & 15);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int h = (lane >> 4) * 4 + i;
        if (h >= G) continue;
        const float sv = sum_smem[h];
        const float inv = sv > 0.0f ? 1.0f / sv : 0.0f;
        out[((long)b * num_q_heads + kvh * G + h) * HEAD_DIM + dim] =
            f2bf(acc_pv[nsub][i] * inv);
      }
    }
  } else {
#pragma unroll
    for (int nsub = 0; nsub < 2; ++nsub) {
      const int dim = 16 * (wave + 4 * nsub) + (lane & 15);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int h = (lane >> 4) * 4 + i;
        if (h >= G) continue;
        float* wsp = workspace +
            ws_row_offset(b, kvh, h, split, num_kv_heads, G, num_splits);
        if (wave == 0 && nsub == 0 && (lane & 15) == 0) {
          wsp[0] = m_smem[h];
          wsp[1] = sum_smem[h];
        }
        wsp[2 + dim] = acc_pv[nsub][i];
      }
    }
  }
}

// Merge split-KV partials: one MERGE_WAVES-wave workgroup per (b, q_head).
// Each wave reduces a strided subset of the splits into a partial
// (m, s, acc[128]), then wave 0 combines the MERGE_WAVES partials through
// LDS. A single-wave merge looping over ~224 splits serially was HALF the
// long-context step time (profiles/longctx_kernel_stats.txt pre-fix:
// 101 µs vs the 115 µs attention sweep).
#define MERGE_WAVES 8
__global__ __launch_bounds__(64 * MERGE_WAVES) void gqa_decode_attn_merge_kernel(
    bf16* __restrict__ out,          // [B, Hq, 128]
    const float* __restrict__ workspace,  // [B, Hk, G, splits, 2+128]
    const int num_q_heads,
    const int num_kv_heads,
    const int num_splits) {
  const int b = blockIdx.x;
  const int h = blockIdx.y;  // query head
  const int G = num_q_heads / num_kv_heads;
  const int kvh = h / G;
  const int g = h % G;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;

  __shared__ float sm_m[MERGE_WAVES];
  __shared__ float sm_s[MERGE_WAVES];
  __shared__ float sm_o[MERGE_WAVES][HEAD_DIM];

  const float* base = workspace +
      ws_row_offset(b, kvh, g, 0, num_kv_heads, G, num_splits);
  // wave-local pass over its strided split subset
  float M = -INFINITY;
  for (int sp = wave; sp < num_splits; sp += MERGE_WAVES) {
    M = fmaxf(M, base[sp * (2 + HEAD_DIM)]);
  }
  float S = 0.0f, o0 = 0.0f, o1 = 0.0f;
  for (int sp = wave; sp < num_splits; sp += MERGE_WAVES) {
    const float* wsp = base + sp * (2 + HEAD_DIM);
    const float mw = wsp[0];
    if (mw == -INFINITY) continue;
    const float f = __expf(mw - M);
    S += wsp[1] * f;
    o0 = fmaf(wsp[2 + 2 * lane], f, o0);
    o1 = fmaf(wsp[2 + 2 * lane + 1], f, o1);
  }
  if (lane == 0) {
    sm_m[wave] = M;
    sm_s[wave] = S;
  }
  sm_o[wave][2 * lane] = o0;
  sm_o[wave][2 * lane + 1] = o1;
  __syncthreads();

  if (wave != 0) return;
  // combine the wave partials (online-softmax merge across MERGE_WAVES
  // terms)
  float Mg = -INFINITY;
  for (int w = 0; w < MERGE_WAVES; ++w) Mg = fmaxf(Mg, sm_m[w]);
  float Sg = 0.0f;
  float g0 = 0.0f, g1 = 0.0f;
  for (int w = 0; w < MERGE_WAVES; ++w) {
    if (sm_m[w] == -INFINITY) continue;
    const float f = __expf(sm_m[w] - Mg);
    Sg += sm_s[w] * f;
    g0 = fmaf(sm_o[w][2 * lane], f, g0);
    g1 = fmaf(sm_o[w][2 * lane + 1], f, g1);
  }
  const float inv = Sg > 0.0f ? 1.0f / Sg : 0.0f;
  bf16x2* orow = reinterpret_cast<bf16x2*>(
      out + ((long)b * num_q_heads + h) * HEAD_DIM);
  orow[lane] = bf16x2{f2bf(g0 * inv), f2bf(g1 * inv)};
}

extern "C" int gqa_decode_attn_num_splits(int batch, int num_kv_heads,
                                          int max_ctx_hint) {
  // Fill the v4 kernel's resident workgroups: 70 VGPRs / ~21 KiB LDS
  // admit 7 WGs/CU (compiler occupancy report) → target ~1792 WGs over
  // 256 CUs, subject to the caps below.
  const int base = batch * num_kv_heads;
  if (base >= 1792) return 1;
  int splits = 1792 / base;
  // Split cap: 16 for moderate contexts (diminishing returns once each
  // split's tile count is small), but LONG contexts lift it — at B=1
  // ctx=128k the 16-split grid is 128 WGs on 256 CUs (7% of resident
  // capacity) and the KV sweep ran at 0.43 TB/s (profiles/
  // longctx_itl.json, pre-fix). Allow as many splits as keep >=
  // min_tiles (default 8) tiles of work per split; the merge kernel's
  // cost is O(splits) per (b,h) row and stays negligible. Whatever the
  // cap, never more splits than pairs of tiles in the context.
  static int min_tiles = [] {
    const char* e = getenv("WVA_ATTN_MIN_TILES");  // tuning knob
    int v = e ? atoi(e) : 8;
    return v > 0 ? v : 8;
  }();
  int cap = 16;
  if (max_ctx_hint > 0) {
    const int by_work = max_ctx_hint / (min_tiles * TILE);
    if (by_work > cap) cap = by_work;
  }
  if (splits > cap) splits = cap;
  const int max_useful = max_ctx_hint > 0 ? (max_ctx_hint + 2 * TILE - 1) / (2 * TILE) : splits;
  if (splits > max_useful && max_useful >= 1) splits = max_useful;
  return splits < 1 ? 1 : splits;
}

// The v4/v5 × bf16/fp8 choice of one layout; all eight instantiations share
// one signature.
template <bool PAGED>
static auto decode_attn_kernel(int variant, int kv_fp8) {
  return variant == 5 ? (kv_fp8 ? gqa_decode_attn_v5_kernel<true, PAGED>
                                : gqa_decode_attn_v5_kernel<false, PAGED>)
                      : (kv_fp8 ? gqa_decode_attn_v4_kernel<true, PAGED>
                                : gqa_decode_attn_v4_kernel<false, PAGED>);
}

extern "C" void launch_gqa_decode_attn(
    void* out, void* workspace, const void* q, const void* k_cache,
    const void* v_cache, const int* context_lens, const PagedKV* paged,
    int batch, int num_q_heads, int num_kv_heads, int max_seq, int num_splits,
    float scale, int variant, int kv_fp8, hipStream_t stream) {
  const auto kernel = !paged ? decode_attn_kernel<false>(variant, kv_fp8)
                             : decode_attn_kernel<true>(variant, kv_fp8);
  const PagedKV p = paged ? *paged : PagedKV{nullptr, 0, 0, 0};
  if (paged) max_seq = p.max_blocks << p.block_shift;
  hipLaunchKernelGGL(kernel, dim3(batch, num_kv_heads, num_splits), dim3(256),
                     0, stream, (bf16*)out, (float*)workspace, (const bf16*)q,
                     k_cache, v_cache, context_lens, num_q_heads, num_kv_heads,
                     max_seq, scale, p.block_tables, p.max_blocks,
                     p.block_shift, p.num_blocks);
  if (num_splits > 1) {
    hipLaunchKernelGGL(gqa_decode_attn_merge_kernel,
                       dim3(batch, num_q_heads), dim3(64 * MERGE_WAVES), 0,
                       stream, (bf16*)out, (const float*)workspace,
                       num_q_heads, num_kv_heads, num_splits);
  }
}
