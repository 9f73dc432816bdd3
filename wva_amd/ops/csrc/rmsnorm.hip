// Fused (add-)RMSNorm for bf16, fp32 accumulation — MI355X (gfx950).
//
// Memory-bound: one read of x (+residual), one write. Vectorized 8-wide
// (4 × bf16x2 = 16 B/lane) so a 256-thread workgroup moves 4 KiB per
// load instruction — the coalescing sweet spot on CDNA4 (guide §2).
// One workgroup per row; rows = batch (decode) or batch×seq (prefill).
// Hidden sizes are multiples of 2048 for the models we serve, so the
// vector path requires H % 8 == 0 (checked host-side).

#include "common.h"
#include "launch.h"

typedef __attribute__((ext_vector_type(4))) float floatx4;

// out = (x + residual?) * rsqrt(mean(x²)+eps) * weight ; residual_out = x+residual
template <bool HAS_RESIDUAL>
__global__ void rmsnorm_kernel(
    bf16* __restrict__ out,
    bf16* __restrict__ residual_out,  // updated in place when HAS_RESIDUAL
    const bf16* __restrict__ input,
    const bf16* __restrict__ residual,
    const bf16* __restrict__ weight,
    const float eps,
    const int hidden) {
  const int row = blockIdx.x;
  const bf16* in_row = input + (long)row * hidden;
  const bf16* res_row = HAS_RESIDUAL ? residual + (long)row * hidden : nullptr;
  bf16* out_row = out + (long)row * hidden;
  bf16* res_out_row =
      HAS_RESIDUAL ? residual_out + (long)row * hidden : nullptr;

  __shared__ float lds_red[16];

  // Pass 1: accumulate sum of squares (and fold residual) in fp32.
  float ss = 0.0f;
  const int vec_n = hidden / 8;
  const bf16x2* in2 = reinterpret_cast<const bf16x2*>(in_row);
  const bf16x2* res2 =
      HAS_RESIDUAL ? reinterpret_cast<const bf16x2*>(res_row) : nullptr;
  bf16x2* res_out2 =
      HAS_RESIDUAL ? reinterpret_cast<bf16x2*>(res_out_row) : nullptr;

  for (int i = threadIdx.x; i < vec_n; i += blockDim.x) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      bf16x2 v = in2[i * 4 + j];
      float lo = bf2f(v.x), hi = bf2f(v.y);
      if (HAS_RESIDUAL) {
        bf16x2 r = res2[i * 4 + j];
        lo += bf2f(r.x);
        hi += bf2f(r.y);
        res_out2[i * 4 + j] = bf16x2{f2bf(lo), f2bf(hi)};
      }
      ss = fmaf(lo, lo, ss);
      ss = fmaf(hi, hi, ss);
    }
  }
  ss = block_reduce_sum(ss, lds_red);
  const float inv_rms = rsqrtf(ss / (float)hidden + eps);
  __syncthreads();

  // Pass 2: normalize and scale. Re-read folded x from residual_out when
  // fused (it stays L2/L1-hot — row is ≤32 KiB), from input otherwise.
  const bf16x2* x2 = HAS_RESIDUAL ? reinterpret_cast<const bf16x2*>(res_out_row)
                                  : in2;
  const bf16x2* w2 = reinterpret_cast<const bf16x2*>(weight);
  bf16x2* o2 = reinterpret_cast<bf16x2*>(out_row);
  for (int i = threadIdx.x; i < vec_n; i += blockDim.x) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      bf16x2 v = x2[i * 4 + j];
      bf16x2 w = w2[i * 4 + j];
      o2[i * 4 + j] = bf16x2{
          f2bf(bf2f(v.x) * inv_rms * bf2f(w.x)),
          f2bf(bf2f(v.y) * inv_rms * bf2f(w.y))};
    }
  }
}

extern "C" void launch_rmsnorm(
    void* out, void* residual_out, const void* input, const void* residual,
    const void* weight, float eps, int rows, int hidden, hipStream_t stream) {
  dim3 grid(rows);
  dim3 block(256);
  if (residual != nullptr) {
    hipLaunchKernelGGL(rmsnorm_kernel<true>, grid, block, 0, stream,
                       (bf16*)out, (bf16*)residual_out, (const bf16*)input,
                       (const bf16*)residual, (const bf16*)weight, eps, hidden);
  } else {
    hipLaunchKernelGGL(rmsnorm_kernel<false>, grid, block, 0, stream,
                       (bf16*)out, nullptr, (const bf16*)input, nullptr,
                       (const bf16*)weight, eps, hidden);
  }
}
