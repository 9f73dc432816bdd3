// Device-side routed MoE expert MLP, decode and prefill — MI355X (gfx950).
//
//   route:    fp32 router logits [T,E] → top-k ids/weights, per-expert
//             offsets and the stable expert-sorted slot list
//   gate_up:  act_sorted[p,:] = silu(g)·u, g/u = x[token(p)] · W_gate_up[e]^T
//   down:     y[p,:] = act_sorted[p,:] · W_down[e]^T  (split-K, fp32
//             partials indexed by slot) + a combine kernel that sums the
//             top-k contributions of each token in a fixed order
//
// Everything a launch needs (grid, workspace) derives from the static
// shapes (T, E, top_k, H, I); routing lives in device tensors the kernels
// read at execution time, so a captured step replays with fresh routing.
// No host reads, no atomics: every output element has exactly one writer
// and every sum has a fixed order, so results are bit-reproducible.
//
// The two GEMMs reuse the skinny_gemm.hip structure — no LDS, no
// barriers; each wave streams its 16-row W tiles from HBM straight into
// MFMA B fragments and re-reads the (L2-resident) A rows — with one level
// of indirection: the m-tile grid dimension is launched at its static
// upper bound min(T·K, T·K/BM + E) and each workgroup finds its
// (expert, m-tile) by scanning expert_offsets. Workgroups past the last
// non-empty tile exit before touching a weight, so an expert with no
// routed rows streams nothing.
//
// That streaming family is the decode shape: a handful of rows per expert.
// Once an expert owns 128 rows and more (prefill) every 64-row m-tile would
// stream the expert again, so a second, compute-shaped family follows it:
// moe_gate_up_swiglu_tiled_kernel and moe_down_tiled_kernel stage 128-row A
// and W tiles through LDS and share them among the four waves (see "tiled
// grouped GEMMs" below). moe_use_tiled picks the family from (T·K, E) alone;
// route, sort and combine are common to both.
//
// The streaming family also takes weight-only fp8 experts (W8A16): e4m3
// weights with one fp32 scale per (expert, output row), bf16 activations and
// the same bf16 MFMA (moe_mma_stream_fp8 and the two *_fp8_kernel). The
// scale is applied once, in fp32, to the accumulator; grids, splits,
// workspace and combine are those of the bf16 call. The tiled family has no
// fp8 form yet: fp8 weights stream at every T.
//
// Fragment convention as in skinny_gemm.hip: identical lane→k bijection
// for A and B (a different one than skinny_gemm's, see moe_mma_stream);
// C/D mapping col = lane&15 (n), row = (lane>>4)·4 + reg (m).

#include "common.h"
#include "launch.h"

#define MOE_KT 128      // K elements per unrolled block
#define MOE_BM 64       // sorted rows per m-tile (4 MFMA m-subtiles)
#define MOE_NT 64       // W rows per workgroup per n-subtile (16 per wave)
#define MOE_MAX_E 64
#define MOE_MAX_K 8

// ---------------------------------------------------------------- route

// One thread per token: top-k by repeated argmax (strict '>' so the lowest
// expert index wins an exact tie), softmax over the k selected logits.
__global__ __launch_bounds__(256) void moe_topk_kernel(
    int* __restrict__ topk_idx,      // [T, K]
    float* __restrict__ topk_w,      // [T, K]
    const float* __restrict__ logits,  // [T, E]
    const int T, const int E, const int K) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= T) return;
  const float* row = logits + (long)t * E;
  unsigned long long taken = 0ull;
  float sel[MOE_MAX_K];
#pragma unroll
  for (int k = 0; k < MOE_MAX_K; ++k) {
    if (k >= K) break;
    int best = -1;
    float best_v = 0.f;
    for (int e = 0; e < E; ++e) {
      if ((taken >> e) & 1ull) continue;
      const float v = row[e];
      if (best < 0 || v > best_v) {
        best = e;
        best_v = v;
      }
    }
    taken |= 1ull << best;  // K <= E: an untaken expert always exists
    sel[k] = best_v;
    topk_idx[(long)t * K + k] = best;
  }
  const float row_max = sel[0];  // selection order is descending
  float denom = 0.f;
#pragma unroll
  for (int k = 0; k < MOE_MAX_K; ++k) {
    if (k >= K) break;
    sel[k] = expf(sel[k] - row_max);
    denom += sel[k];
  }
#pragma unroll
  for (int k = 0; k < MOE_MAX_K; ++k) {
    if (k >= K) break;
    topk_w[(long)t * K + k] = sel[k] / denom;
  }
}

// Stable counting sort of the n = T·K slots by expert, one workgroup.
// Thread i owns the contiguous slot range [i·chunk, (i+1)·chunk); for each
// expert a block-wide exclusive scan of the per-thread match counts gives
// every thread its write position, so slots stay ascending inside an
// expert group. E block scans of 256 counters — microseconds at decode
// sizes, and still only n·E/256 loads per thread at prefill sizes.
__global__ __launch_bounds__(256) void moe_sort_kernel(
    int* __restrict__ expert_offsets,  // [E + 1]
    int* __restrict__ sorted_slots,    // [n]
    const int* __restrict__ topk_idx,  // [n]
    const int n, const int E) {
  __shared__ int wave_total[4];
  const int tid = threadIdx.x;
  const int lane = tid & (WAVE_SIZE - 1);
  const int wave = tid / WAVE_SIZE;
  const int chunk = (n + 255) / 256;
  const int c0 = min(n, tid * chunk);
  const int c1 = min(n, c0 + chunk);
  int base = 0;
  for (int e = 0; e < E; ++e) {
    int cnt = 0;
    for (int s = c0; s < c1; ++s) cnt += (topk_idx[s] == e) ? 1 : 0;
    int incl = cnt;
#pragma unroll
    for (int d = 1; d < WAVE_SIZE; d <<= 1) {
      const int v = __shfl_up(incl, d, WAVE_SIZE);
      if (lane >= d) incl += v;
    }
    if (lane == WAVE_SIZE - 1) wave_total[wave] = incl;
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const int v = wave_total[w];
      if (w < wave) before += v;
      total += v;
    }
    __syncthreads();
    if (tid == 0) expert_offsets[e] = base;
    int pos = base + before + incl - cnt;
    for (int s = c0; s < c1; ++s) {
      if (topk_idx[s] == e && pos < n) sorted_slots[pos++] = s;
    }
    base += total;
  }
  if (tid == 0) expert_offsets[E] = base;
}

// ------------------------------------------------------- grouped GEMMs

struct MoeTile {
  int expert;
  int row0;  // first sorted position of this m-tile
  int rows;  // live rows, 1..BM
};

// Map a linear m-tile index onto (expert, m-tile within expert) for m-tiles
// of BM sorted rows. Uniform across the workgroup (scalar loads); false =
// past the last live tile.
template <int BM>
__device__ __forceinline__ bool moe_find_tile(
    const int* __restrict__ expert_offsets, const int E, int tile,
    MoeTile& out) {
  int begin = expert_offsets[0];
  for (int e = 0; e < E; ++e) {
    const int end = expert_offsets[e + 1];
    const int n_e = end - begin;
    const int tiles_e = (n_e + BM - 1) / BM;
    if (tile < tiles_e && begin >= 0) {
      out.expert = e;
      out.row0 = begin + tile * BM;
      out.rows = min(BM, n_e - tile * BM);
      return true;
    }
    tile -= tiles_e;
    begin = end;
  }
  return false;
}

// Stream K-range [k_begin, k_end) of NSUB 16-row W tiles against up to
// four 16-row A subtiles. a_rows/w_rows are this lane's row pointers
// (always in bounds); dead rows fold into zero fragments.
template <int NSUB>
__device__ __forceinline__ void moe_mma_stream(
    moe_f32x4 (&acc)[4][NSUB], const bf16* const (&a_rows)[4],
    const bool (&a_live)[4], const bf16* const (&w_rows)[NSUB],
    const bool (&n_live)[NSUB], const int mt, const int k_begin,
    const int k_end, const int lane) {
  // Lane→k bijection (shared by A and B, so any choice is exact): k-group
  // g = lane/16 reads the 8 elements at 32·kk + 8·g, i.e. the four lanes
  // that share a W row read one contiguous 64 B run per load instruction.
  // skinny_gemm's choice (each LANE contiguous across kk, 16 B pieces 64 B
  // apart within an instruction) measured 2.9 vs 4.6 TB/s here.
  const int lane_k = 8 * (lane / 16);
  // Workgroups start at staggered K blocks and wrap, so the chip is not
  // reading the same 256 B-aligned column of every W row at one time
  // (rows are a power-of-two stride apart in gate_up); +3-5% measured.
  const int nkb = (k_end - k_begin) / MOE_KT;
  int kb = (int)((blockIdx.x * 5 + blockIdx.y * 3) % nkb);
  for (int it = 0; it < nkb; ++it) {
    const int k0 = k_begin + kb * MOE_KT;
    if (++kb == nkb) kb = 0;
#pragma unroll
    for (int kk = 0; kk < MOE_KT / 32; ++kk) {
      const int k = k0 + 32 * kk + lane_k;
      moe_bf16x8 b_frag[NSUB];
#pragma unroll
      for (int ns = 0; ns < NSUB; ++ns) {
        if (n_live[ns]) {
          b_frag[ns] = *reinterpret_cast<const moe_bf16x8*>(w_rows[ns] + k);
        } else {
#pragma unroll
          for (int i = 0; i < 8; ++i) b_frag[ns][i] = 0;
        }
      }
#pragma unroll
      for (int pm = 0; pm < 4; ++pm) {
        if (pm >= mt) break;
        moe_bf16x8 a_frag;
        if (a_live[pm]) {
          a_frag = *reinterpret_cast<const moe_bf16x8*>(a_rows[pm] + k);
        } else {
#pragma unroll
          for (int i = 0; i < 8; ++i) a_frag[i] = 0;
        }
#pragma unroll
        for (int ns = 0; ns < NSUB; ++ns) {
          acc[pm][ns] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              a_frag, b_frag[ns], acc[pm][ns], 0, 0, 0);
        }
      }
    }
  }
}

// moe_mma_stream for weight-only fp8 (W8A16): W rows are e4m3 bytes, A rows
// stay bf16, the MFMA is the same bf16 one. The bf16 lane→k map on 1-byte
// elements would shrink the run that the four lanes of a W row read per
// load instruction to 32 B. So the 128-k block is walked as two halves of
// 64 k instead, and in half j k-group g = lane/16 owns the SIXTEEN elements
// at 64·j + 16·g: W is one 16-byte load per live row — again one contiguous
// 64 B run per row and instruction, with half as many load instructions per
// block — and A the 16 bf16 at the same k as two adjacent 16-byte loads.
// Elements 0..7 feed one MFMA and 8..15 the next, for A and B alike, so the
// k-sum is exact as before. The raw e4m3 values are multiplied; the row
// scale commutes with the k-sum and is the caller's epilogue.
template <int NSUB>
__device__ __forceinline__ void moe_mma_stream_fp8(
    moe_f32x4 (&acc)[4][NSUB], const bf16* const (&a_rows)[4],
    const bool (&a_live)[4], const fp8_t* const (&w_rows)[NSUB],
    const bool (&n_live)[NSUB], const int mt, const int k_begin,
    const int k_end, const int lane) {
  const int lane_k = 16 * (lane / 16);
  // the staggered, wrapping K start of moe_mma_stream
  const int nkb = (k_end - k_begin) / MOE_KT;
  int kb = (int)((blockIdx.x * 5 + blockIdx.y * 3) % nkb);
  for (int it = 0; it < nkb; ++it) {
    const int k0 = k_begin + kb * MOE_KT;
    if (++kb == nkb) kb = 0;
#pragma unroll
    for (int j = 0; j < MOE_KT / 64; ++j) {
      const int k = k0 + 64 * j + lane_k;
      uint4 wq[NSUB];
#pragma unroll
      for (int ns = 0; ns < NSUB; ++ns) {
        // e4m3 zero is the zero byte: a dead row converts to a zero fragment
        wq[ns] = n_live[ns] ? *reinterpret_cast<const uint4*>(w_rows[ns] + k)
                            : make_uint4(0u, 0u, 0u, 0u);
      }
      // one 8-element half at a time, so that only one converted B fragment
      // per n-subtile is live next to the raw bytes of the other half
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        moe_bf16x8 b_frag[NSUB];
#pragma unroll
        for (int ns = 0; ns < NSUB; ++ns) {
          b_frag[ns] = h == 0 ? fp8x8_to_bf16x8(wq[ns].x, wq[ns].y)
                              : fp8x8_to_bf16x8(wq[ns].z, wq[ns].w);
        }
#pragma unroll
        for (int pm = 0; pm < 4; ++pm) {
          if (pm >= mt) break;
          moe_bf16x8 a_frag;
          if (a_live[pm]) {
            a_frag =
                *reinterpret_cast<const moe_bf16x8*>(a_rows[pm] + k + 8 * h);
          } else {
#pragma unroll
            for (int i = 0; i < 8; ++i) a_frag[i] = 0;
          }
#pragma unroll
          for (int ns = 0; ns < NSUB; ++ns) {
            acc[pm][ns] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                a_frag, b_frag[ns], acc[pm][ns], 0, 0, 0);
          }
        }
      }
    }
  }
}

// act_sorted[p, n] = silu(g)·u with g = x[token(p)]·Wg[e][n], u = ...Wu[e][n].
// Each wave owns 16 gate rows AND the matching 16 up rows (offset I) of
// the stacked [E, 2I, H] weight, both multiplied against the same
// gathered A fragments, so SwiGLU runs on the accumulators in registers.
// grid = (ceil(I/64), m_tiles).
__global__ __launch_bounds__(256, 2) void moe_gate_up_swiglu_kernel(
    bf16* __restrict__ act,               // [T*K, I]
    const bf16* __restrict__ x,           // [T, H]
    const bf16* __restrict__ w,           // [E, 2I, H]
    const int* __restrict__ expert_offsets,
    const int* __restrict__ sorted_slots,
    const int T, const int E, const int top_k, const int H, const int I) {
  MoeTile tile;
  if (!moe_find_tile<MOE_BM>(expert_offsets, E, blockIdx.y, tile)) return;
  const int lane = threadIdx.x & (WAVE_SIZE - 1);
  const int wave = threadIdx.x / WAVE_SIZE;
  const int n0 = blockIdx.x * MOE_NT + 16 * wave;
  if (n0 >= I) return;  // I % 16 == 0: a wave's tile is all live or dead
  const int TK = T * top_k;

  const bf16* w_e = w + (long)tile.expert * 2 * I * H;
  const bf16* w_rows[2];
  w_rows[0] = w_e + (long)(n0 + (lane & 15)) * H;
  w_rows[1] = w_rows[0] + (long)I * H;
  const bool n_live[2] = {true, true};

  const int mt = (tile.rows + 15) / 16;
  const bf16* a_rows[4];
  bool a_live[4];
#pragma unroll
  for (int pm = 0; pm < 4; ++pm) {
    const int m = pm * 16 + (lane & 15);
    const int p = tile.row0 + m;
    a_live[pm] = m < tile.rows && p < TK;
    // the gather: sorted position → slot → token row of x
    const int slot = a_live[pm] ? sorted_slots[p] : 0;
    const int token = min(max(slot / top_k, 0), T - 1);
    a_rows[pm] = x + (long)token * H;
  }

  moe_f32x4 acc[4][2];
#pragma unroll
  for (int pm = 0; pm < 4; ++pm)
#pragma unroll
    for (int ns = 0; ns < 2; ++ns)
      acc[pm][ns] = moe_f32x4{0.f, 0.f, 0.f, 0.f};

  moe_mma_stream<2>(acc, a_rows, a_live, w_rows, n_live, mt, 0, H, lane);

  const int n_out = n0 + (lane & 15);
#pragma unroll
  for (int pm = 0; pm < 4; ++pm) {
    if (pm >= mt) break;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int m = pm * 16 + (lane >> 4) * 4 + i;
      const int p = tile.row0 + m;
      if (m >= tile.rows || p >= TK) continue;
      const float g = acc[pm][0][i];
      const float u = acc[pm][1][i];
      act[(long)p * I + n_out] = f2bf(g / (1.0f + expf(-g)) * u);
    }
  }
}

// moe_gate_up_swiglu_kernel for e4m3 weights with one fp32 scale per (expert,
// stacked row), w_scale [E, 2I]: same grid, tile search, gather and SwiGLU. A
// lane's output column is fixed, so it loads its gate and its up scale once,
// before the K loop, and applies them in fp32 to the accumulators ahead of
// SwiGLU. (Written out next to the bf16 kernel instead of sharing one
// templated body with it: routed through a shared body the bf16 kernel no
// longer compiled to the instructions it was measured with.)
__global__ NO_PACKED_FP32 __launch_bounds__(256, 2) void
moe_gate_up_swiglu_fp8_kernel(
    bf16* __restrict__ act,               // [T*K, I]
    const bf16* __restrict__ x,           // [T, H]
    const fp8_t* __restrict__ w,          // [E, 2I, H] e4m3
    const float* __restrict__ w_scale,    // [E, 2I]
    const int* __restrict__ expert_offsets,
    const int* __restrict__ sorted_slots,
    const int T, const int E, const int top_k, const int H, const int I) {
  MoeTile tile;
  if (!moe_find_tile<MOE_BM>(expert_offsets, E, blockIdx.y, tile)) return;
  const int lane = threadIdx.x & (WAVE_SIZE - 1);
  const int wave = threadIdx.x / WAVE_SIZE;
  const int n0 = blockIdx.x * MOE_NT + 16 * wave;
  if (n0 >= I) return;  // I % 16 == 0: a wave's tile is all live or dead
  const int TK = T * top_k;
  const int n_out = n0 + (lane & 15);

  const fp8_t* w_rows[2];
  w_rows[0] = w + ((long)tile.expert * 2 * I + n_out) * H;
  w_rows[1] = w_rows[0] + (long)I * H;
  const bool n_live[2] = {true, true};
  const float* scale_e = w_scale + (long)tile.expert * 2 * I + n_out;
  const float scale_g = scale_e[0];
  const float scale_u = scale_e[I];

  const int mt = (tile.rows + 15) / 16;
  const bf16* a_rows[4];
  bool a_live[4];
#pragma unroll
  for (int pm = 0; pm < 4; ++pm) {
    const int m = pm * 16 + (lane & 15);
    const int p = tile.row0 + m;
    a_live[pm] = m < tile.rows && p < TK;
    // the gather: sorted position → slot → token row of x
    const int slot = a_live[pm] ? sorted_slots[p] : 0;
    const int token = min(max(slot / top_k, 0), T - 1);
    a_rows[pm] = x + (long)token * H;
  }

  moe_f32x4 acc[4][2];
#pragma unroll
  for (int pm = 0; pm < 4; ++pm)
#pragma unroll
    for (int ns = 0; ns < 2; ++ns)
      acc[pm][ns] = moe_f32x4{0.f, 0.f, 0.f, 0.f};

  moe_mma_stream_fp8<2>(acc, a_rows, a_live, w_rows, n_live, mt, 0, H, lane);

#pragma unroll
  for (int pm = 0; pm < 4; ++pm) {
    if (pm >= mt) break;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int m = pm * 16 + (lane >> 4) * 4 + i;
      const int p = tile.row0 + m;
      if (m >= tile.rows || p >= TK) continue;
      const float g = scale_g * acc[pm][0][i];
      const float u = scale_u * acc[pm][1][i];
      act[(long)p * I + n_out] = f2bf(g / (1.0f + expf(-g)) * u);
    }
  }
}

// Split-K partial of y[p, :] = act_sorted[p, :] · W_down[e]^T, written to
// ws[sk][slot(p)][:] — indexed by SLOT so the combine kernel reads each
// token's top-k contributions at fixed addresses. Every slot belongs to
// exactly one (expert, m-tile), so each ws row has one writer per split.
// grid = (ceil(H/(64·NSUB)), m_tiles, SK).
template <int NSUB>
__global__ __launch_bounds__(256, 2) void moe_down_kernel(
    float* __restrict__ ws,               // [SK, T*K, H]
    const bf16* __restrict__ act,         // [T*K, I]
    const bf16* __restrict__ w,           // [E, H, I]
    const int* __restrict__ expert_offsets,
    const int* __restrict__ sorted_slots,
    const int TK, const int E, const int H, const int I) {
  MoeTile tile;
  if (!moe_find_tile<MOE_BM>(expert_offsets, E, blockIdx.y, tile)) return;
  const int lane = threadIdx.x & (WAVE_SIZE - 1);
  const int wave = threadIdx.x / WAVE_SIZE;
  const int sk = blockIdx.z;
  const int SK = gridDim.z;
  const int n0 = blockIdx.x * MOE_NT * NSUB + 16 * NSUB * wave;
  if (n0 >= H) return;  // H % 16 == 0

  const bf16* w_e = w + (long)tile.expert * H * I;
  const bf16* w_rows[NSUB];
  bool n_live[NSUB];
#pragma unroll
  for (int ns = 0; ns < NSUB; ++ns) {
    const int n_row = n0 + 16 * ns + (lane & 15);
    n_live[ns] = n_row < H;
    w_rows[ns] = w_e + (long)(n_live[ns] ? n_row : 0) * I;
  }

  const int mt = (tile.rows + 15) / 16;
  const bf16* a_rows[4];
  bool a_live[4];
#pragma unroll
  for (int pm = 0; pm < 4; ++pm) {
    const int m = pm * 16 + (lane & 15);
    const int p = tile.row0 + m;
    a_live[pm] = m < tile.rows && p < TK;
    a_rows[pm] = act + (long)(a_live[pm] ? p : 0) * I;
  }

  moe_f32x4 acc[4][NSUB];
#pragma unroll
  for (int pm = 0; pm < 4; ++pm)
#pragma unroll
    for (int ns = 0; ns < NSUB; ++ns)
      acc[pm][ns] = moe_f32x4{0.f, 0.f, 0.f, 0.f};

  const int chunks_per_split = (I / MOE_KT) / SK;
  const int k_begin = sk * chunks_per_split * MOE_KT;
  moe_mma_stream<NSUB>(acc, a_rows, a_live, w_rows, n_live, mt, k_begin,
                       k_begin + chunks_per_split * MOE_KT, lane);

#pragma unroll
  for (int pm = 0; pm < 4; ++pm) {
    if (pm >= mt) break;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int m = pm * 16 + (lane >> 4) * 4 + i;
      const int p = tile.row0 + m;
      if (m >= tile.rows || p >= TK) continue;
      const int slot = sorted_slots[p];
      if (slot < 0 || slot >= TK) continue;
      float* dst = ws + ((long)sk * TK + slot) * H;
#pragma unroll
      for (int ns = 0; ns < NSUB; ++ns) {
        const int n_out = n0 + 16 * ns + (lane & 15);
        if (n_out < H) dst[n_out] = acc[pm][ns][i];
      }
    }
  }
}

// moe_down_kernel for e4m3 weights with w_scale [E, H]: same grid, splits and
// workspace rows. The partial stored to ws is scale·acc (a row scale commutes
// with the k-sum), so moe_combine_kernel and its sum order do not change. A
// dead column takes scale 0 and, as there, is not stored.
template <int NSUB>
__global__ NO_PACKED_FP32 __launch_bounds__(256, 2) void moe_down_fp8_kernel(
    float* __restrict__ ws,               // [SK, T*K, H]
    const bf16* __restrict__ act,         // [T*K, I]
    const fp8_t* __restrict__ w,          // [E, H, I] e4m3
    const float* __restrict__ w_scale,    // [E, H]
    const int* __restrict__ expert_offsets,
    const int* __restrict__ sorted_slots,
    const int TK, const int E, const int H, const int I) {
  MoeTile tile;
  if (!moe_find_tile<MOE_BM>(expert_offsets, E, blockIdx.y, tile)) return;
  const int lane = threadIdx.x & (WAVE_SIZE - 1);
  const int wave = threadIdx.x / WAVE_SIZE;
  const int sk = blockIdx.z;
  const int SK = gridDim.z;
  const int n0 = blockIdx.x * MOE_NT * NSUB + 16 * NSUB * wave;
  if (n0 >= H) return;  // H % 16 == 0

  const fp8_t* w_rows[NSUB];
  bool n_live[NSUB];
  float scale[NSUB];
#pragma unroll
  for (int ns = 0; ns < NSUB; ++ns) {
    const int n_row = n0 + 16 * ns + (lane & 15);
    n_live[ns] = n_row < H;
    const long row = (long)tile.expert * H + (n_live[ns] ? n_row : 0);
    w_rows[ns] = w + row * I;
    scale[ns] = n_live[ns] ? w_scale[row] : 0.f;
  }

  const int mt = (tile.rows + 15) / 16;
  const bf16* a_rows[4];
  bool a_live[4];
#pragma unroll
  for (int pm = 0; pm < 4; ++pm) {
    const int m = pm * 16 + (lane & 15);
    const int p = tile.row0 + m;
    a_live[pm] = m < tile.rows && p < TK;
    a_rows[pm] = act + (long)(a_live[pm] ? p : 0) * I;
  }

  moe_f32x4 acc[4][NSUB];
#pragma unroll
  for (int pm = 0; pm < 4; ++pm)
#pragma unroll
    for (int ns = 0; ns < NSUB; ++ns)
      acc[pm][ns] = moe_f32x4{0.f, 0.f, 0.f, 0.f};

  const int chunks_per_split = (I / MOE_KT) / SK;
  const int k_begin = sk * chunks_per_split * MOE_KT;
  moe_mma_stream_fp8<NSUB>(acc, a_rows, a_live, w_rows, n_live, mt, k_begin,
                           k_begin + chunks_per_split * MOE_KT, lane);

#pragma unroll
  for (int pm = 0; pm < 4; ++pm) {
    if (pm >= mt) break;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int m = pm * 16 + (lane >> 4) * 4 + i;
      const int p = tile.row0 + m;
      if (m >= tile.rows || p >= TK) continue;
      const int slot = sorted_slots[p];
      if (slot < 0 || slot >= TK) continue;
      float* dst = ws + ((long)sk * TK + slot) * H;
#pragma unroll
      for (int ns = 0; ns < NSUB; ++ns) {
        const int n_out = n0 + 16 * ns + (lane & 15);
        if (n_out < H) dst[n_out] = scale[ns] * acc[pm][ns][i];
      }
    }
  }
}

// out[t, :] = bf16(Σ_k topk_w[t,k] · Σ_sk ws[sk][t·K + k][:]) — the
// inverted index is just the slot id, and both sums run in a fixed order.
// One thread per 4 output columns.
__global__ __launch_bounds__(256) void moe_combine_kernel(
    bf16* __restrict__ out,            // [T, H]
    const float* __restrict__ ws,      // [SK, T*K, H]
    const float* __restrict__ topk_w,  // [T, K]
    const int T, const int K, const int H, const int SK) {
  const int h4 = H / 4;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)T * h4) return;
  const int t = (int)(i / h4);
  const int n = (int)(i % h4) * 4;
  const long TK = (long)T * K;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (int k = 0; k < K; ++k) {
    const long slot = (long)t * K + k;
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    for (int sk = 0; sk < SK; ++sk) {
      const float4 v =
          *reinterpret_cast<const float4*>(ws + (sk * TK + slot) * H + n);
      s[0] += v.x;
      s[1] += v.y;
      s[2] += v.z;
      s[3] += v.w;
    }
    const float wk = topk_w[slot];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] += wk * s[j];
  }
  bf16* dst = out + (long)t * H + n;
#pragma unroll
  for (int j = 0; j < 4; ++j) dst[j] = f2bf(acc[j]);
}

// ------------------------------------------------- tiled grouped GEMMs
//
// The compute-shaped family for many rows per expert. One workgroup of four
// waves owns 128 sorted rows × 128 W rows of one expert and walks K in steps
// of 64. Per step all 256 threads stage the A tile (128 × 64 bf16) and the W
// tile (128 × 64 bf16) into LDS with 16-byte global loads; the waves, laid
// out 2 × 2, read their MFMA fragments from there. So a W element is fetched
// from memory once per 128 rows (the streaming kernels: once per 64) and an
// A element once per workgroup (there: once per wave and n-tile).
//
// Schedule: two LDS buffers, one barrier per step. The global loads of step
// k+1 are issued into registers before the MFMAs of step k and committed to
// the other buffer after them; the barrier that ends step k both publishes
// that buffer and retires the reads of step k's. (One buffer would need a
// second barrier per step between the last fragment read and the commit.)
//
// Dead rows — A rows past tile.rows or with p ≥ T·K, W rows past the last
// column — are never loaded: their staging registers stay zero and zeros go
// to LDS. Their row pointer is row 0 of an in-bounds block and is not
// dereferenced; a token index is clamped into [0, T-1] as in the streaming
// kernel.

#define MOE_TBM 128     // sorted rows per tiled m-tile (2 waves × 4 subtiles)
#define MOE_TBN 128     // W rows per tiled workgroup (2 waves × 4 subtiles)
#define MOE_TBK 64      // K elements staged per step (2 MFMA k-steps)
// LDS row stride in dwords: 32 of data (64 bf16) + 4 of pad = 144 bytes, so
// every 16-byte access stays aligned. Fragment read (ds_read_b128): lane l
// reads the 4 dwords at 36·row + 16·kk + 4·(l >> 4), row = subtile base +
// (l & 15). A subtile base is a multiple of 16 rows = 576 dwords = 9·64, no
// bank shift. The 16 lanes of one k-group start at banks 36·r mod 64 = 0,
// 36, 8, 44, 16, 52, 24, 60, 32, 4, 40, 12, 48, 20, 56, 28 for r = 0..15:
// 36 = 4·9 with 9 odd, so r → 9r mod 16 is a bijection and the sixteen
// 4-dword runs tile the 64 banks exactly once — conflict-free; the same
// holds for any 8 consecutive rows on 32 banks. Without the pad (stride 32)
// rows r and r + 2 would share their banks, an 8-way conflict.
// Staging write (ds_write_b128): thread t writes chunk t & 7 of row t >> 3,
// so 16 lanes cover two rows, banks [0, 32) and [36, 68) mod 64: one chunk
// in sixteen meets a 2-way conflict, which is accepted.
#define MOE_TROW_DW 36
#define MOE_TTILE_DW (128 * MOE_TROW_DW)   // one 128-row tile
#define MOE_TBUF_DW (2 * MOE_TTILE_DW)     // A tile + W tile
#define MOE_TLDS_DW (2 * MOE_TBUF_DW)      // two buffers: 73728 bytes

// K loop of one tiled workgroup. Thread t stages chunk t & 7 (8 bf16) of the
// tile rows (t >> 3) + 32·j, j = 0..3, of A and of W: a_src / w_src point at
// that chunk at k = 0 (always in bounds), *_live says whether the row is
// loaded at all. Wave (wm, wn) accumulates tile rows 64·wm .. + 64 against
// four 16-row W subtiles: LDS W rows 64·wn + 16·ns of a plain tile (down),
// or, when the tile stacks 64 gate rows on the matching 64 up rows
// (GATE_UP), gate rows 32·wn + 16·(ns & 1) for ns < 2 and the same up rows
// (+ 64) for ns ≥ 2. mt = live 16-row A subtiles of this wave (0..4).
template <bool GATE_UP>
__device__ __forceinline__ void moe_tiled_mainloop(
    moe_f32x4 (&acc)[4][4], const bf16* const (&a_src)[4],
    const bool (&a_live)[4], const bf16* const (&w_src)[4],
    const bool (&w_live)[4], const int kdim, const int mt,
    unsigned int* lds) {
  const int tid = threadIdx.x;
  const int lane = tid & (WAVE_SIZE - 1);
  const int wm = tid / (2 * WAVE_SIZE);
  const int wn = (tid / WAVE_SIZE) & 1;

  uint4 ra[4], rw[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    ra[j] = make_uint4(0u, 0u, 0u, 0u);
    rw[j] = make_uint4(0u, 0u, 0u, 0u);
  }
  auto fetch = [&](const int k0) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (a_live[j]) ra[j] = *reinterpret_cast<const uint4*>(a_src[j] + k0);
      if (w_live[j]) rw[j] = *reinterpret_cast<const uint4*>(w_src[j] + k0);
    }
  };
  const int stage_dw = (tid >> 3) * MOE_TROW_DW + (tid & 7) * 4;
  auto commit = [&](unsigned int* buf) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      unsigned int* dst = buf + stage_dw + 32 * j * MOE_TROW_DW;
      *reinterpret_cast<uint4*>(dst) = ra[j];
      *reinterpret_cast<uint4*>(dst + MOE_TTILE_DW) = rw[j];
    }
  };

  // same lane→k bijection for A and B: k-group lane/16 of each 32-k step
  const int frag_dw = (lane & 15) * MOE_TROW_DW + (lane >> 4) * 4;
  const int a_dw = 64 * wm * MOE_TROW_DW + frag_dw;
  int w_dw[4];
#pragma unroll
  for (int ns = 0; ns < 4; ++ns) {
    const int w_row = GATE_UP ? 64 * (ns >> 1) + 32 * wn + 16 * (ns & 1)
                              : 64 * wn + 16 * ns;
    w_dw[ns] = MOE_TTILE_DW + w_row * MOE_TROW_DW + frag_dw;
  }

  fetch(0);
  commit(lds);
  __syncthreads();
  const int nk = kdim / MOE_TBK;
  for (int kb = 0; kb < nk; ++kb) {
    const unsigned int* cur = lds + (kb & 1) * MOE_TBUF_DW;
    const bool more = kb + 1 < nk;  // uniform
    if (more) fetch((kb + 1) * MOE_TBK);
#pragma unroll
    for (int kk = 0; kk < MOE_TBK / 32; ++kk) {
      moe_bf16x8 b_frag[4];
#pragma unroll
      for (int ns = 0; ns < 4; ++ns) {
        b_frag[ns] =
            *reinterpret_cast<const moe_bf16x8*>(cur + w_dw[ns] + 16 * kk);
      }
#pragma unroll
      for (int pm = 0; pm < 4; ++pm) {
        if (pm >= mt) break;
        const moe_bf16x8 a_frag = *reinterpret_cast<const moe_bf16x8*>(
            cur + a_dw + 16 * pm * MOE_TROW_DW + 16 * kk);
#pragma unroll
        for (int ns = 0; ns < 4; ++ns) {
          acc[pm][ns] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              a_frag, b_frag[ns], acc[pm][ns], 0, 0, 0);
        }
      }
    }
    if (more) commit(lds + ((kb + 1) & 1) * MOE_TBUF_DW);
    __syncthreads();
  }
}

// The tiled gate_up + SwiGLU: tile = 128 sorted rows × 64 act columns, i.e.
// 64 gate rows (LDS W rows 0..63) and the matching 64 up rows (64..127) of
// the stacked [E, 2I, H] weight, so SwiGLU runs on the accumulators exactly
// as in moe_gate_up_swiglu_kernel. grid = (ceil(I/64), tiled m_tiles).
__global__ NO_PACKED_FP32 __launch_bounds__(256, 2) void
moe_gate_up_swiglu_tiled_kernel(
    bf16* __restrict__ act,               // [T*K, I]
    const bf16* __restrict__ x,           // [T, H]
    const bf16* __restrict__ w,           // [E, 2I, H]
    const int* __restrict__ expert_offsets,
    const int* __restrict__ sorted_slots,
    const int T, const int E, const int top_k, const int H, const int I) {
  MoeTile tile;
  if (!moe_find_tile<MOE_TBM>(expert_offsets, E, blockIdx.y, tile)) return;
  __shared__ __attribute__((aligned(16))) unsigned int lds[MOE_TLDS_DW];
  const int tid = threadIdx.x;
  const int lane = tid & (WAVE_SIZE - 1);
  const int wm = tid / (2 * WAVE_SIZE);
  const int wn = (tid / WAVE_SIZE) & 1;
  const int n0 = blockIdx.x * (MOE_TBN / 2);  // < I by the grid
  const int TK = T * top_k;

  const bf16* w_e = w + (long)tile.expert * 2 * I * H;
  const int c8 = (tid & 7) * 8;
  const bf16* a_src[4];
  const bf16* w_src[4];
  bool a_live[4], w_live[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int r = (tid >> 3) + 32 * j;
    const int p = tile.row0 + r;
    a_live[j] = r < tile.rows && p < TK;
    // the gather: sorted position → slot → token row of x
    const int slot = a_live[j] ? sorted_slots[p] : 0;
    const int token = min(max(slot / top_k, 0), T - 1);
    a_src[j] = x + (long)token * H + c8;
    const int n = n0 + (r & 63);
    w_live[j] = n < I;
    w_src[j] = w_e + ((long)(w_live[j] ? n : 0) + (r >= 64 ? I : 0)) * H + c8;
  }

  moe_f32x4 acc[4][4];
#pragma unroll
  for (int pm = 0; pm < 4; ++pm)
#pragma unroll
    for (int ns = 0; ns < 4; ++ns)
      acc[pm][ns] = moe_f32x4{0.f, 0.f, 0.f, 0.f};

  const int mt = min(max((tile.rows - 64 * wm + 15) / 16, 0), 4);
  moe_tiled_mainloop<true>(acc, a_src, a_live, w_src, w_live, H, mt, lds);

#pragma unroll
  for (int pm = 0; pm < 4; ++pm) {
    if (pm >= mt) break;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int m = 64 * wm + 16 * pm + (lane >> 4) * 4 + i;
      const int p = tile.row0 + m;
      if (m >= tile.rows || p >= TK) continue;
#pragma unroll
      for (int ns = 0; ns < 2; ++ns) {
        const int n_out = n0 + 32 * wn + 16 * ns + (lane & 15);
        if (n_out >= I) continue;  // I % 16 == 0: uniform per subtile
        const float g = acc[pm][ns][i];
        const float u = acc[pm][2 + ns][i];
        act[(long)p * I + n_out] = f2bf(g / (1.0f + expf(-g)) * u);
      }
    }
  }
}

// The tiled down GEMM: tile = 128 sorted rows × 128 columns of H, K over I,
// no gather (act is already sorted), no split-K: fp32 rows go to
// ws[slot(p)] and moe_combine_kernel runs with SK = 1, so the sum order is
// fixed. grid = (ceil(H/128), tiled m_tiles).
__global__ NO_PACKED_FP32 __launch_bounds__(256, 2) void
moe_down_tiled_kernel(
    float* __restrict__ ws,               // [T*K, H]
    const bf16* __restrict__ act,         // [T*K, I]
    const bf16* __restrict__ w,           // [E, H, I]
    const int* __restrict__ expert_offsets,
    const int* __restrict__ sorted_slots,
    const int TK, const int E, const int H, const int I) {
  MoeTile tile;
  if (!moe_find_tile<MOE_TBM>(expert_offsets, E, blockIdx.y, tile)) return;
  __shared__ __attribute__((aligned(16))) unsigned int lds[MOE_TLDS_DW];
  const int tid = threadIdx.x;
  const int lane = tid & (WAVE_SIZE - 1);
  const int wm = tid / (2 * WAVE_SIZE);
  const int wn = (tid / WAVE_SIZE) & 1;
  const int n0 = blockIdx.x * MOE_TBN;  // < H by the grid

  const bf16* w_e = w + (long)tile.expert * H * I;
  const int c8 = (tid & 7) * 8;
  const bf16* a_src[4];
  const bf16* w_src[4];
  bool a_live[4], w_live[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int r = (tid >> 3) + 32 * j;
    const int p = tile.row0 + r;
    a_live[j] = r < tile.rows && p < TK;
    a_src[j] = act + (long)(a_live[j] ? p : 0) * I + c8;
    const int n = n0 + r;
    w_live[j] = n < H;
    w_src[j] = w_e + (long)(w_live[j] ? n : 0) * I + c8;
  }

  moe_f32x4 acc[4][4];
#pragma unroll
  for (int pm = 0; pm < 4; ++pm)
#pragma unroll
    for (int ns = 0; ns < 4; ++ns)
      acc[pm][ns] = moe_f32x4{0.f, 0.f, 0.f, 0.f};

  const int mt = min(max((tile.rows - 64 * wm + 15) / 16, 0), 4);
  moe_tiled_mainloop<false>(acc, a_src, a_live, w_src, w_live, I, mt, lds);

#pragma unroll
  for (int pm = 0; pm < 4; ++pm) {
    if (pm >= mt) break;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int m = 64 * wm + 16 * pm + (lane >> 4) * 4 + i;
      const int p = tile.row0 + m;
      if (m >= tile.rows || p >= TK) continue;
      const int slot = sorted_slots[p];
      if (slot < 0 || slot >= TK) continue;
      float* dst = ws + (long)slot * H;
#pragma unroll
      for (int ns = 0; ns < 4; ++ns) {
        const int n_out = n0 + 64 * wn + 16 * ns + (lane & 15);
        if (n_out < H) dst[n_out] = acc[pm][ns][i];
      }
    }
  }
}

// ------------------------------------------------------------ launchers

// Static upper bound on non-empty m-tiles: Σ_e ceil(n_e/BM) ≤ TK/BM + E
// (one partial tile per expert at most) and ≤ TK (a tile holds ≥ 1 row).
extern "C" int moe_num_m_tiles(int TK, int E) {
  const int bound = TK / MOE_BM + E;
  return TK < bound ? TK : bound;
}

// The same bound for the 128-row m-tiles of the tiled kernels.
extern "C" int moe_num_m_tiles_tiled(int TK, int E) {
  const int bound = TK / MOE_TBM + E;
  return TK < bound ? TK : bound;
}

// Which family a call with no forced variant runs: tiled once the experts
// own MOE_TILED_MIN_ROWS sorted rows each on average. Static shapes only.
// Never below 128 rows per expert (less than one full tiled m-tile each);
// above that the threshold is the measured one, see docs/mi355x-kernels.md
// "Tiled grouped GEMMs" and profiles/moe_tiled_ab.json.
#define MOE_TILED_MIN_ROWS 128
extern "C" int moe_use_tiled(int TK, int E) {
  return (long)TK >= (long)MOE_TILED_MIN_ROWS * E ? 1 : 0;
}

// n-subtiles per wave in the down GEMM: 2 once an expert can own more
// than one 16-row A subtile (halves the L2 A-read : HBM W-read ratio).
extern "C" int moe_down_nsub(int TK) { return TK > 16 ? 2 : 1; }

// Split-K for the down GEMM (N = H is small): fill ≈1792 workgroups at
// the static m-tile bound; power of two ≤ 16 dividing I/KT.
extern "C" int moe_down_num_splits(int TK, int E, int H, int I) {
  const int nt = MOE_NT * moe_down_nsub(TK);
  const int wgs = ((H + nt - 1) / nt) * moe_num_m_tiles(TK, E);
  const int k_chunks = I / MOE_KT;
  int sk = 1;
  while (sk < 16 && (long)wgs * sk * 2 <= 1792 && (k_chunks % (sk * 2)) == 0) {
    sk *= 2;
  }
  return sk;
}

extern "C" void launch_moe_route(int* topk_idx, float* topk_w,
                                 int* expert_offsets, int* sorted_slots,
                                 const float* logits, int T, int E, int K,
                                 hipStream_t stream) {
  hipLaunchKernelGGL(moe_topk_kernel, dim3((T + 255) / 256), dim3(256), 0,
                     stream, topk_idx, topk_w, logits, T, E, K);
  hipLaunchKernelGGL(moe_sort_kernel, dim3(1), dim3(256), 0, stream,
                     expert_offsets, sorted_slots, topk_idx, T * K, E);
}

extern "C" void launch_moe_gate_up_swiglu(void* act, const void* x,
                                          const void* w,
                                          const float* w_scale, int w_fp8,
                                          const int* expert_offsets,
                                          const int* sorted_slots, int T,
                                          int E, int top_k, int H, int I,
                                          int tiled, hipStream_t stream) {
  if (w_fp8) {  // streaming family only: the caller refuses fp8 + tiled
    dim3 grid((I + MOE_NT - 1) / MOE_NT, moe_num_m_tiles(T * top_k, E));
    hipLaunchKernelGGL(moe_gate_up_swiglu_fp8_kernel, grid, dim3(256), 0,
                       stream, (bf16*)act, (const bf16*)x, (const fp8_t*)w,
                       w_scale, expert_offsets, sorted_slots, T, E, top_k, H,
                       I);
    return;
  }
  if (tiled) {
    dim3 grid((I + MOE_TBN / 2 - 1) / (MOE_TBN / 2),
              moe_num_m_tiles_tiled(T * top_k, E));
    hipLaunchKernelGGL(moe_gate_up_swiglu_tiled_kernel, grid, dim3(256), 0,
                       stream, (bf16*)act, (const bf16*)x, (const bf16*)w,
                       expert_offsets, sorted_slots, T, E, top_k, H, I);
    return;
  }
  dim3 grid((I + MOE_NT - 1) / MOE_NT, moe_num_m_tiles(T * top_k, E));
  hipLaunchKernelGGL(moe_gate_up_swiglu_kernel, grid, dim3(256), 0, stream,
                     (bf16*)act, (const bf16*)x, (const bf16*)w,
                     expert_offsets, sorted_slots, T, E, top_k, H, I);
}

// tiled: num_splits must be 1 (the tiled kernel does not split K).
extern "C" void launch_moe_down_combine(void* out, float* ws,
                                        const void* act, const void* w,
                                        const float* w_scale, int w_fp8,
                                        const float* topk_w,
                                        const int* expert_offsets,
                                        const int* sorted_slots, int T,
                                        int E, int top_k, int H, int I,
                                        int num_splits, int tiled,
                                        hipStream_t stream) {
  const int TK = T * top_k;
  if (w_fp8) {  // streaming family only, same grid as the bf16 call
    tiled = 0;
    const int nsub = moe_down_nsub(TK);
    const int nt = MOE_NT * nsub;
    dim3 grid((H + nt - 1) / nt, moe_num_m_tiles(TK, E), num_splits);
    if (nsub == 1) {
      hipLaunchKernelGGL((moe_down_fp8_kernel<1>), grid, dim3(256), 0, stream,
                         ws, (const bf16*)act, (const fp8_t*)w, w_scale,
                         expert_offsets, sorted_slots, TK, E, H, I);
    } else {
      hipLaunchKernelGGL((moe_down_fp8_kernel<2>), grid, dim3(256), 0, stream,
                         ws, (const bf16*)act, (const fp8_t*)w, w_scale,
                         expert_offsets, sorted_slots, TK, E, H, I);
    }
  } else if (tiled) {
    dim3 grid((H + MOE_TBN - 1) / MOE_TBN, moe_num_m_tiles_tiled(TK, E));
    hipLaunchKernelGGL(moe_down_tiled_kernel, grid, dim3(256), 0, stream, ws,
                       (const bf16*)act, (const bf16*)w, expert_offsets,
                       sorted_slots, TK, E, H, I);
  } else {
    const int nsub = moe_down_nsub(TK);
    const int nt = MOE_NT * nsub;
    dim3 grid((H + nt - 1) / nt, moe_num_m_tiles(TK, E), num_splits);
    if (nsub == 1) {
      hipLaunchKernelGGL((moe_down_kernel<1>), grid, dim3(256), 0, stream, ws,
                         (const bf16*)act, (const bf16*)w, expert_offsets,
                         sorted_slots, TK, E, H, I);
    } else {
      hipLaunchKernelGGL((moe_down_kernel<2>), grid, dim3(256), 0, stream, ws,
                         (const bf16*)act, (const bf16*)w, expert_offsets,
                         sorted_slots, TK, E, H, I);
    }
  }
  const long n4 = (long)T * (H / 4);
  hipLaunchKernelGGL(moe_combine_kernel, dim3((n4 + 255) / 256), dim3(256),
                     0, stream, (bf16*)out, (const float*)ws, topk_w, T,
                     top_k, H, tiled ? 1 : num_splits);
}
