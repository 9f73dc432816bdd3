// Causal flash-attention forward for PREFILL — MI355X (gfx950).
//
// Shape contract: head_dim = 128, GQA G = Hq/Hk ≤ 8, one query TILE of
// 64 positions per workgroup: grid = (B·Hq, ceil(S/64)). Each of the 4
// waves OWNS 16 query rows (one 16-row m-tile), so the online softmax
// needs no cross-wave communication at all; K/V tiles are shared
// through L2 (K) and LDS (V).
//
// Per (q-tile i, kv-tile j) iteration, per wave:
//   * S_ij [16q × 64k]: 4 n-tiles × 4 k-subtiles of
//     mfma_f32_16x16x32_bf16 — A = Q fragments (persistent, loaded once
//     per workgroup), B = K fragments streamed straight from the
//     head-major cache (HBM→VGPR, the v4-scores pattern; the G-way
//     reuse across q-head workgroups is served by L2).
//   * causal mask + online softmax on the accumulator fragments: row
//     max/sum are 16-lane shuffle reductions (a C/D row lives in one
//     16-lane group, one register).
//   * P staged to LDS (bf16), V staged to LDS (cooperative, like v3/v5);
//     O_i [16q × 128d] += P·V as 2 k-subtiles × 8 dim-tiles of MFMA with
//     B = V fragments from LDS u16 reads (the v5-PV pattern).
// Causality at tile granularity: kv-tile j is processed only while
// j·64 ≤ i·64 + 63; the diagonal tile applies the per-element mask.
//
// Layouts match the decode path: q [T, Hq, 128] (T = B·S, row-major
// tokens), k/v head-major caches [B, Hk, S_max, 128] (ALREADY populated
// by the caller for positions < S), out [T, Hq, 128].
//
// Fragment conventions probe-verified in scripts/mfma_probe.hip; the
// C/D mapping is col = lane&15, row = (lane>>4)·4 + reg.

#include "common.h"
#include "launch.h"

#define HEAD_DIM 128
#define QT 64              // query rows per workgroup
#define KT_POS 64          // kv positions per tile
#define NUM_WAVES 4
#define ROW_DW 66          // LDS dword stride for V rows (64 + 2 pad)
#define P_ROW 66           // LDS stride for P rows (64 positions + pad)

__device__ __forceinline__ float group16_max(float v) {
  // max across the 16-lane group holding one C/D row
#pragma unroll
  for (int off = 8; off > 0; off >>= 1) {
    v = fmaxf(v, __shfl_xor(v, off, WAVE_SIZE));
  }
  return v;
}

__device__ __forceinline__ float group16_sum(float v) {
#pragma unroll
  for (int off = 8; off > 0; off >>= 1) {
    v += __shfl_xor(v, off, WAVE_SIZE);
  }
  return v;
}

// HAS_PREFIX (chunked prefill, "extend"): the S query rows of sequence b
// are a chunk that sits at absolute positions P_b .. P_b+S-1, with
// P_b = prefix_lens[b] read on the device; the caches already hold the
// prefix and the chunk's own rows. Query i sees key kp iff kp <= P_b + i.
// The kv tiles stay aligned at 0, so a row goes through the same tile
// sequence however the prompt was chunked; the q-tile is then unaligned to
// them and its diagonal may cross two tiles, which the per-element mask
// (applied on every tile) covers. P_b and the live row count are clamped
// to the slab, so no content of prefix_lens can take a load out of it.
// Without HAS_PREFIX, P_b is the constant 0 and the kernel is the
// one-shot prefill.
//
// RAGGED (implies HAS_PREFIX): q/out are packed [T, Hq, 128] and sequence b
// owns the len_b = chunk_lens[b] rows from q_starts[b]; S is only the static
// upper bound of len_b that sized the grid, so a workgroup whose q-tile
// starts at or past len_b returns, and the live cache rows end at
// P_b + len_b. blockIdx.z is a split of the kv sweep: split s of N walks
// the tiles s, s+N, s+2N, ... below the q-tile's own kv_end (the decode
// kernels' interleaving; it balances whatever the lengths are). N == 1
// stores the normalised output as the other modes do; N > 1 stores the
// unnormalised (m, s, o[128]) of every live row to `ws` for
// extend_ragged_merge_kernel. len_b, q_starts[b] and P_b are clamped, so
// no content of a device tensor takes a load or a store out of its buffer.
#define WS_ROW (2 + HEAD_DIM)  // floats of one (row, head, split) partial

// chunk_lens[b] clamped to [0, min(max_chunk, T)]
__device__ __forceinline__ int ragged_len(const int* chunk_lens, int b,
                                          int max_chunk, int total_rows) {
  return min(max(chunk_lens[b], 0), min(max_chunk, total_rows));
}

// q_starts[b] clamped to [0, T - len_b]
__device__ __forceinline__ int ragged_start(const int* q_starts, int b,
                                            int len_b, int total_rows) {
  return min(max(q_starts[b], 0), total_rows - len_b);
}

// first float of the partial of row r (0..63) of q-tile `tile` of (b, h)
// = bh, split `split` of `num_splits`; `tiles` = ceil(max_chunk / 64)
__device__ __forceinline__ long ragged_ws_off(int bh, int tiles, int tile,
                                              int r, int num_splits,
                                              int split) {
  return ((((long)bh * tiles + tile) * QT + r) * num_splits + split) * WS_ROW;
}

template <bool KV_FP8, bool HAS_PREFIX, bool RAGGED = false>
__global__ __launch_bounds__(256, 2) void prefill_attn_kernel(
    bf16* __restrict__ out,            // [T, Hq, 128]
    const bf16* __restrict__ q,        // [T, Hq, 128]
    const void* __restrict__ k_cache,  // [B, Hk, S_max, 128] bf16|e4m3
    const void* __restrict__ v_cache,
    const int* __restrict__ prefix_lens,  // [B], HAS_PREFIX only
    const int B,
    const int S,                       // query rows per sequence
    const int num_q_heads,
    const int num_kv_heads,
    const int max_seq,
    const float scale,
    const int* __restrict__ q_starts,    // [B], RAGGED only
    const int* __restrict__ chunk_lens,  // [B], RAGGED only
    float* __restrict__ ws,              // partials, RAGGED with splits > 1
    const int total_rows) {              // T, RAGGED only
  static_assert(HAS_PREFIX || !RAGGED, "RAGGED implies HAS_PREFIX");
  const int bh = blockIdx.x;           // b * Hq + h
  const int b = bh / num_q_heads;
  const int h = bh % num_q_heads;
  const int kvh = h / (num_q_heads / num_kv_heads);
  const int qt0 = blockIdx.y * QT;     // first query position of the tile
  // query rows of sequence b (S is their static bound when RAGGED) and
  // the first of them in q/out
  int S_b = S;
  int row0 = b * S;
  if constexpr (RAGGED) {
    S_b = ragged_len(chunk_lens, b, S, total_rows);
    row0 = ragged_start(q_starts, b, S_b, total_rows);
  }
  if (qt0 >= S_b) return;

  // first absolute position of the chunk, and rows of the slab that are
  // live (prefix + chunk); rows at or past kv_len may hold anything
  int q_pos0 = 0;
  int kv_len = S_b;
  if constexpr (HAS_PREFIX) {
    q_pos0 = min(max(prefix_lens[b], 0), max_seq);
    kv_len = min(q_pos0 + S_b, max_seq);
  }
  // this workgroup's share of the kv tiles: all of them unless RAGGED
  int kt_first = 0;
  int kt_step = KT_POS;
  if constexpr (RAGGED) {
    kt_first = blockIdx.z * KT_POS;
    kt_step = gridDim.z * KT_POS;
  }

  const int lane = threadIdx.x & (WAVE_SIZE - 1);
  const int wave = threadIdx.x / WAVE_SIZE;

  // V staged TRANSPOSED: [dim][pos] u16 rows (stride 68 = 64 + 4 pad:
  // 2·row mod 32 is distinct for the 16 rows of a fragment read, so the
  // b64 pairs are bank-conflict-free). A B-fragment (k = 8 consecutive
  // positions at fixed dim) is then one contiguous 16 B row segment
  // instead of 8 scattered u16 reads.
#define VT_ROW 68
  __shared__ unsigned short v_smem_t[HEAD_DIM * VT_ROW];
  __shared__ float p_smem[NUM_WAVES][16][P_ROW];

  const long slab_off = ((long)b * num_kv_heads + kvh) * max_seq * HEAD_DIM;
  const bf16* k_slab = reinterpret_cast<const bf16*>(k_cache) + slab_off;
  const fp8_t* k_slab8 = reinterpret_cast<const fp8_t*>(k_cache) + slab_off;
  const unsigned int* v_base = reinterpret_cast<const unsigned int*>(
      reinterpret_cast<const bf16*>(v_cache) + slab_off);
  const fp8_t* v_base8 = reinterpret_cast<const fp8_t*>(v_cache) + slab_off;

  // --- persistent Q fragments for this wave's 16 rows ---
  // A-frag: lane row = q-row (l%16), k = head-dim 8·(l/16)+i, 4 subtiles
  const int my_q = qt0 + 16 * wave + (lane % 16);  // global q position
  const bool q_live = my_q < S_b;
  bf16x8_frag q_frag[4];
  {
    const int col0 = 8 * (lane / 16);
    if (q_live) {
      const short* qrow = reinterpret_cast<const short*>(
          q + ((long)(row0 + my_q) * num_q_heads + h) * HEAD_DIM);
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        q_frag[kk] =
            *reinterpret_cast<const bf16x8_frag*>(qrow + 32 * kk + col0);
      }
    } else {
#pragma unroll
      for (int kk = 0; kk < 4; ++kk)
#pragma unroll
        for (int i = 0; i < 8; ++i) q_frag[kk][i] = 0;
    }
  }

  // online-softmax state per owned q-row: the row for C/D reg i is
  // r = (lane>>4)·4 + i; every lane in a 16-lane group carries the same
  // 4 rows, so m/s are per (reg) and uniform across the group after
  // reductions.
  float m_run[4], s_run[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    m_run[i] = -INFINITY;
    s_run[i] = 0.0f;
  }
  // O accumulators: 8 dim-tiles × f32x4 (C/D row = q-row, col = dim)
  f32x4_frag o_acc[8];
#pragma unroll
  for (int n = 0; n < 8; ++n) o_acc[n] = f32x4_frag{0.f, 0.f, 0.f, 0.f};

  // causal upper bound of this q-tile's sweep
  const int kv_end = min(q_pos0 + qt0 + QT, kv_len);

  for (int kt0 = kt_first; kt0 < kv_end; kt0 += kt_step) {
    const int kn = min(KT_POS, kv_len - kt0);

    // --- stage V tile transposed (cooperative, all waves): each
    // thread reads one dim-pair at one position (coalesced along the
    // HBM row) and scatters two bf16 u16s into dim-major rows; the fp8
    // path up-converts here so downstream fragments are unchanged ---
    if constexpr (KV_FP8) {
      const fp8_t* v_src = v_base8 + (long)kt0 * HEAD_DIM;
      const int total = kn * (HEAD_DIM / 2);  // byte-pairs in the tile
      for (int idx = wave * WAVE_SIZE + lane; idx < total;
           idx += NUM_WAVES * WAVE_SIZE) {
        const int pos = idx >> 6;          // 64 pairs per position row
        const int d2 = idx & 63;
        const unsigned short packed = *reinterpret_cast<const unsigned short*>(
            v_src + (long)pos * HEAD_DIM + 2 * d2);
        const float2_vt f = unpk2_fp8(packed);
        const bf16 b0 = f2bf(f[0]);
        const bf16 b1 = f2bf(f[1]);
        v_smem_t[(2 * d2) * VT_ROW + pos] =
            *reinterpret_cast<const unsigned short*>(&b0);
        v_smem_t[(2 * d2 + 1) * VT_ROW + pos] =
            *reinterpret_cast<const unsigned short*>(&b1);
      }
    } else {
      const unsigned int* v_src = &v_base[(long)kt0 * (HEAD_DIM / 2)];
      const int total = kn * (HEAD_DIM / 2);  // dwords in the tile
      for (int idx = wave * WAVE_SIZE + lane; idx < total;
           idx += NUM_WAVES * WAVE_SIZE) {
        const int pos = idx >> 6;          // 64 dwords per position row
        const int d2 = idx & 63;           // dim pair
        const unsigned int val = v_src[idx];
        v_smem_t[(2 * d2) * VT_ROW + pos] = (unsigned short)(val & 0xffffu);
        v_smem_t[(2 * d2 + 1) * VT_ROW + pos] =
            (unsigned short)(val >> 16);
      }
    }

    // --- scores S_ij: 4 n-tiles × 4 k-subtiles ---
    f32x4_frag s_frag[4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) s_frag[nt] = f32x4_frag{0.f, 0.f, 0.f, 0.f};
    {
      const int col0 = 8 * (lane / 16);
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        const int kpos = kt0 + 16 * nt + (lane % 16);
        const int kpos_c = kpos < max_seq ? kpos : max_seq - 1;
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
          bf16x8_frag k_frag;
          if constexpr (KV_FP8) {
            const unsigned short* src =
                reinterpret_cast<const unsigned short*>(
                    k_slab8 + (long)kpos_c * HEAD_DIM + 32 * kk + col0);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const float2_vt f = unpk2_fp8(src[j]);
              k_frag[2 * j] = f2bf_bits(f[0]);
              k_frag[2 * j + 1] = f2bf_bits(f[1]);
            }
          } else {
            const short* krow = reinterpret_cast<const short*>(
                k_slab + (long)kpos_c * HEAD_DIM);
            k_frag =
                *reinterpret_cast<const bf16x8_frag*>(krow + 32 * kk + col0);
          }
          s_frag[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              q_frag[kk], k_frag, s_frag[nt], 0, 0, 0);
        }
      }
    }

    // --- causal mask + online softmax on the fragments ---
    // element (reg i, n-tile nt): q-row r = qt0 + 16·wave + (lane>>4)·4+i
    // at absolute position q_pos0 + r, k-pos = kt0 + 16·nt + (lane&15)
    float tile_max[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) tile_max[i] = -INFINITY;
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int qr = qt0 + 16 * wave + (lane >> 4) * 4 + i;
        const int kp = kt0 + 16 * nt + (lane & 15);
        float v = s_frag[nt][i] * scale;
        if (kp > q_pos0 + qr || kp >= kn + kt0 || qr >= S_b) v = -INFINITY;
        s_frag[nt][i] = v;
        tile_max[i] = fmaxf(tile_max[i], v);
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) tile_max[i] = group16_max(tile_max[i]);

    float corr[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float m_new = fmaxf(m_run[i], tile_max[i]);
      corr[i] = (m_run[i] == -INFINITY) ? 0.0f : __expf(m_run[i] - m_new);
      m_run[i] = m_new;
    }
    float tile_sum[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float p = (s_frag[nt][i] == -INFINITY)
                            ? 0.0f
                            : __expf(s_frag[nt][i] - m_run[i]);
        s_frag[nt][i] = p;
        tile_sum[i] += p;
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      s_run[i] = s_run[i] * corr[i] + group16_sum(tile_sum[i]);
    }

    // rescale O by corr (per q-row = per reg)
#pragma unroll
    for (int n = 0; n < 8; ++n)
#pragma unroll
      for (int i = 0; i < 4; ++i) o_acc[n][i] *= corr[i];

    // --- stage P to this wave's LDS pane (bf16 would do; fp32 keeps
    // the write simple and the A-frag build cheap) ---
    // element (reg i, nt) → row (lane>>4)·4+i, col 16·nt + (lane&15)
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
#pragma unroll
      for (int i = 0; i < 4; ++i)
        p_smem[wave][(lane >> 4) * 4 + i][16 * nt + (lane & 15)] =
            s_frag[nt][i];

    __syncthreads();  // V staged + P visible (own pane only, but V needs it)

    // --- O += P·V: A = P (row = q-row, k = positions), B = V from the
    // transposed LDS tile (one contiguous row segment per fragment) ---
    {
      const bool full = (kn == KT_POS);
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {  // 2 position subtiles of 32
        bf16x8_frag p_frag;
        {
          const int row = lane % 16;
          const int p0 = 32 * kk + 8 * (lane / 16);
#pragma unroll
          for (int i = 0; i < 8; ++i)
            p_frag[i] = f2bf_bits(p_smem[wave][row][p0 + i]);
        }
#pragma unroll
        for (int n = 0; n < 8; ++n) {
          const int dim = 16 * n + (lane % 16);
          const int p0 = 32 * kk + 8 * (lane / 16);
          bf16x8_frag v_frag;
          const unsigned short* vrow = &v_smem_t[dim * VT_ROW + p0];
          if (full) {
#pragma unroll
            for (int i = 0; i < 8; ++i) v_frag[i] = (short)vrow[i];
          } else {
#pragma unroll
            for (int i = 0; i < 8; ++i)
              v_frag[i] = (p0 + i < kn) ? (short)vrow[i] : (short)0;
          }
          o_acc[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              p_frag, v_frag, o_acc[n], 0, 0, 0);
        }
      }
    }
    __syncthreads();  // done with V before the next tile restages
  }

  // --- split sweep: the unnormalised partial of every live row; a split
  // that met no tile stores m = -inf, s = 0, o = 0 ---
  if constexpr (RAGGED) {
    if (gridDim.z > 1) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int r = 16 * wave + (lane >> 4) * 4 + i;
        if (qt0 + r >= S_b) continue;
        float* wrow = ws + ragged_ws_off(bh, gridDim.y, blockIdx.y, r,
                                         gridDim.z, blockIdx.z);
        if ((lane & 15) == 0) {
          wrow[0] = m_run[i];
          wrow[1] = s_run[i];
        }
#pragma unroll
        for (int n = 0; n < 8; ++n)
          wrow[2 + 16 * n + (lane & 15)] = o_acc[n][i];
      }
      return;
    }
  }

  // --- write O / s normalization: element (reg i, dim-tile n):
  // q-row = qt0 + 16·wave + (lane>>4)·4 + i, dim = 16·n + (lane&15) ---
#pragma unroll
  for (int n = 0; n < 8; ++n) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int qr = qt0 + 16 * wave + (lane >> 4) * 4 + i;
      if (qr >= S_b) continue;
      const float inv = s_run[i] > 0.0f ? 1.0f / s_run[i] : 0.0f;
      out[((long)(row0 + qr) * num_q_heads + h) * HEAD_DIM + 16 * n +
          (lane & 15)] = f2bf(o_acc[n][i] * inv);
    }
  }
}

// Merge of the split sweep: out row = sum_s exp(m_s - m) o_s / sum_s
// exp(m_s - m) s_s with m = max_s m_s. Grid (B·Hq, ceil(max_chunk/64), 16):
// a wave per row (4 rows per workgroup), a lane per dim pair; the m_s are
// read a lane each and max-reduced, the partials of the splits are
// independent loads. Splits with m = -inf met no visible key and are
// skipped; a row all of whose splits are empty is written as zeros. Lengths
// and starts are clamped exactly as in the attention kernel, so the same
// rows are read as were written.
#define MERGE_ROWS 4  // rows (= waves) per merge workgroup
__global__ __launch_bounds__(64 * MERGE_ROWS) void extend_ragged_merge_kernel(
    bf16* __restrict__ out,              // [T, Hq, 128]
    const float* __restrict__ ws,
    const int* __restrict__ q_starts,    // [B]
    const int* __restrict__ chunk_lens,  // [B]
    const int max_chunk,
    const int num_q_heads,
    const int num_splits,
    const int total_rows) {
  const int bh = blockIdx.x;
  const int b = bh / num_q_heads;
  const int h = bh % num_q_heads;
  const int len_b = ragged_len(chunk_lens, b, max_chunk, total_rows);
  const int row0 = ragged_start(q_starts, b, len_b, total_rows);
  const int lane = threadIdx.x & (WAVE_SIZE - 1);
  const int r = MERGE_ROWS * blockIdx.z + threadIdx.x / WAVE_SIZE;  // 0..63
  const int qr = blockIdx.y * QT + r;
  if (qr >= len_b) return;
  const float* wrow =
      ws + ragged_ws_off(bh, gridDim.y, blockIdx.y, r, num_splits, 0);
  float m = -INFINITY;
  for (int s = lane; s < num_splits; s += WAVE_SIZE)
    m = fmaxf(m, wrow[s * WS_ROW]);
  m = wave_reduce_max(m);
  float sum = 0.0f, o0 = 0.0f, o1 = 0.0f;
#pragma unroll 4
  for (int s = 0; s < num_splits; ++s) {
    const float* wsp = wrow + s * WS_ROW;
    const float m_s = wsp[0];
    const float f = (m_s == -INFINITY) ? 0.0f : __expf(m_s - m);
    const float2 o = *reinterpret_cast<const float2*>(wsp + 2 + 2 * lane);
    sum = fmaf(wsp[1], f, sum);
    o0 = fmaf(o.x, f, o0);
    o1 = fmaf(o.y, f, o1);
  }
  const float inv = sum > 0.0f ? 1.0f / sum : 0.0f;
  bf16x2* orow = reinterpret_cast<bf16x2*>(
      out + ((long)(row0 + qr) * num_q_heads + h) * HEAD_DIM);
  orow[lane] = bf16x2{f2bf(o0 * inv), f2bf(o1 * inv)};
}

template <bool HAS_PREFIX>
static void launch_prefill_kernel(
    void* out, const void* q, const void* k_cache, const void* v_cache,
    const int* prefix_lens, int batch, int rows, int num_q_heads,
    int num_kv_heads, int max_seq, float scale, int kv_fp8,
    hipStream_t stream) {
  dim3 grid(batch * num_q_heads, (rows + QT - 1) / QT);
  dim3 block(256);
  if (kv_fp8) {
    hipLaunchKernelGGL((prefill_attn_kernel<true, HAS_PREFIX>), grid, block,
                       0, stream, (bf16*)out, (const bf16*)q, k_cache,
                       v_cache, prefix_lens, batch, rows, num_q_heads,
                       num_kv_heads, max_seq, scale, nullptr, nullptr,
                       nullptr, 0);
  } else {
    hipLaunchKernelGGL((prefill_attn_kernel<false, HAS_PREFIX>), grid, block,
                       0, stream, (bf16*)out, (const bf16*)q, k_cache,
                       v_cache, prefix_lens, batch, rows, num_q_heads,
                       num_kv_heads, max_seq, scale, nullptr, nullptr,
                       nullptr, 0);
  }
}

extern "C" void launch_prefill_attn(
    void* out, const void* q, const void* k_cache, const void* v_cache,
    const int* prefix_lens, int batch, int rows, int num_q_heads,
    int num_kv_heads, int max_seq, float scale, int kv_fp8,
    hipStream_t stream) {
  if (!prefix_lens) {
    launch_prefill_kernel<false>(out, q, k_cache, v_cache, nullptr, batch,
                                 rows, num_q_heads, num_kv_heads, max_seq,
                                 scale, kv_fp8, stream);
  } else {
    launch_prefill_kernel<true>(out, q, k_cache, v_cache, prefix_lens, batch,
                                rows, num_q_heads, num_kv_heads, max_seq,
                                scale, kv_fp8, stream);
  }
}

// Split count of the ragged extend launch from static shapes only (the
// lengths live on the device). The kernel is resident at 3 waves/SIMD, i.e.
// 3 workgroups per CU or 768 on 256 CUs: once the q-tiles alone fill those
// slots the sweep is not split. Below that each workgroup walks its tiles
// alone at ~6 us per tile and splitting pays until the launch has about
// 2048 workgroups (measured, profiles/ragged_extend_ab.json: 8 splits at
// 256 q-tile workgroups, 16 at 128, still gaining at 24 for 32), with at
// most RAGGED_MAX_SPLITS, the largest count measured, and never more than
// pairs of tiles in max_seq. The workspace needs no cap of its own: base x
// splits <= 2048 bounds it at 2048 x 64 x 130 floats = 68 MB.
#define RAGGED_FILL_WGS 768
#define RAGGED_SPLIT_WGS 2048
#define RAGGED_MAX_SPLITS 24
extern "C" int extend_attn_ragged_num_splits(int batch, int num_q_heads,
                                             int max_chunk, int max_seq) {
  const long base = (long)batch * num_q_heads * ((max_chunk + QT - 1) / QT);
  if (base < 1 || base >= RAGGED_FILL_WGS) return 1;
  int splits = (int)(RAGGED_SPLIT_WGS / base);
  if (splits > RAGGED_MAX_SPLITS) splits = RAGGED_MAX_SPLITS;
  const int max_useful = (max_seq + 2 * KT_POS - 1) / (2 * KT_POS);
  if (splits > max_useful) splits = max_useful;
  return splits < 1 ? 1 : splits;
}

extern "C" void launch_extend_attn_ragged(
    void* out, void* ws, const void* q, const void* k_cache,
    const void* v_cache, const int* prefix_lens, const int* q_starts,
    const int* chunk_lens, int batch, int total_rows, int max_chunk,
    int num_q_heads, int num_kv_heads, int max_seq, int num_splits,
    float scale, int kv_fp8, hipStream_t stream) {
  const auto kernel = kv_fp8 ? prefill_attn_kernel<true, true, true>
                             : prefill_attn_kernel<false, true, true>;
  const dim3 grid(batch * num_q_heads, (max_chunk + QT - 1) / QT, num_splits);
  hipLaunchKernelGGL(kernel, grid, dim3(256), 0, stream, (bf16*)out,
                     (const bf16*)q, k_cache, v_cache, prefix_lens, batch,
                     max_chunk, num_q_heads, num_kv_heads, max_seq, scale,
                     q_starts, chunk_lens, (float*)ws, total_rows);
  if (num_splits > 1) {
    hipLaunchKernelGGL(extend_ragged_merge_kernel,
                       dim3(grid.x, grid.y, QT / MERGE_ROWS),
                       dim3(64 * MERGE_ROWS), 0, stream, (bf16*)out,
                       (const float*)ws,
                       q_starts, chunk_lens, max_chunk, num_q_heads,
                       num_splits, total_rows);
  }
}
