// Device-side routed MoE expert MLP for decode — MI355X (gfx950).
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
  int rows;  // live rows, 1..MOE_BM
};

// Map a linear m-tile index onto (expert, m-tile within expert). Uniform
// across the workgroup (scalar loads); false = past the last live tile.
__device__ __forceinline__ bool moe_find_tile(
    const int* __restrict__ expert_offsets, const int E, int tile,
    MoeTile& out) {
  int begin = expert_offsets[0];
  for (int e = 0; e < E; ++e) {
    const int end = expert_offsets[e + 1];
    const int n_e = end - begin;
    const int tiles_e = (n_e + MOE_BM - 1) / MOE_BM;
    if (tile < tiles_e && begin >= 0) {
      out.expert = e;
      out.row0 = begin + tile * MOE_BM;
      out.rows = min(MOE_BM, n_e - tile * MOE_BM);
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
  if (!moe_find_tile(expert_offsets, E, blockIdx.y, tile)) return;
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
  if (!moe_find_tile(expert_offsets, E, blockIdx.y, tile)) return;
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

// ------------------------------------------------------------ launchers

// Static upper bound on non-empty m-tiles: Σ_e ceil(n_e/BM) ≤ TK/BM + E
// (one partial tile per expert at most) and ≤ TK (a tile holds ≥ 1 row).
extern "C" int moe_num_m_tiles(int TK, int E) {
  const int bound = TK / MOE_BM + E;
  return TK < bound ? TK : bound;
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
                                          const int* expert_offsets,
                                          const int* sorted_slots, int T,
                                          int E, int top_k, int H, int I,
                                          hipStream_t stream) {
  dim3 grid((I + MOE_NT - 1) / MOE_NT, moe_num_m_tiles(T * top_k, E));
  hipLaunchKernelGGL(moe_gate_up_swiglu_kernel, grid, dim3(256), 0, stream,
                     (bf16*)act, (const bf16*)x, (const bf16*)w,
                     expert_offsets, sorted_slots, T, E, top_k, H, I);
}

extern "C" void launch_moe_down_combine(void* out, float* ws,
                                        const void* act, const void* w,
                                        const float* topk_w,
                                        const int* expert_offsets,
                                        const int* sorted_slots, int T,
                                        int E, int top_k, int H, int I,
                                        int num_splits,
                                        hipStream_t stream) {
  const int TK = T * top_k;
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
  const long n4 = (long)T * (H / 4);
  hipLaunchKernelGGL(moe_combine_kernel, dim3((n4 + 255) / 256), dim3(256),
                     0, stream, (bf16*)out, (const float*)ws, topk_w, T,
                     top_k, H, num_splits);
}
