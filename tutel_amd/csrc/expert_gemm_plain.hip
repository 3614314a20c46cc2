// expert_gemm_plain.hip -- the PLAIN instantiations of the 128 x 256 ring tile (gemm_big_tile<.., PLAIN = true>, gemm_dev.h), one
// (expert, N-tile) per workgroup, and their launcher.  A translation unit of its own: expert_gemm.hip already takes minutes to compile.
// Which launches take it: gemm_plain_admits (gemm_plan.hip) under TUTEL_AMD_GEMM_PLAIN.  What is different from
// expert_gemm_big_kernel<T, true, ACT, 4, 3, true, 128, FL> is only what surrounds the K loop (gemm_plain.h): same bits.
#include "gemm_dev.h"

// The argument block arrives in one batch (gemm_plain_fetch_args, gemm_dev.h); one M-tile per expert, so work item w = e * ntn + nt.
template <typename T, int ACT, bool FL>
__global__ __launch_bounds__(256, 2) void expert_gemm_plain_kernel(GemmPlainArgs) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const GemmPlainArgs p = gemm_plain_fetch_args();
  const uint32_t w = (uint32_t)xcd_work_item(p.grid), e = gemm_plain_div(w, (uint32_t)p.ntn, p.rcp_ntn);
  gemm_big_tile<T, true, ACT, 4, 3, true, 128, FL, GemmNoHook, true>(p, (int)e, 0, (int)(w - e * (uint32_t)p.ntn), smem);
}

using GemmPlainKernel = void (*)(GemmPlainArgs);
int tutel_gemm_plain_launch(const GemmPlan &pl, const GemmArgs &a, int dtype, int act, hipStream_t st) {
  const GemmPlainArgs p = gemm_plain_pack(a, pl.ntn, pl.grid);
  return dispatch_dtype_act<TUTEL_ACT_NONE, TUTEL_ACT_RELU, TUTEL_ACT_GELU, TUTEL_ACT_SILU>(
      dtype, act,
      [&](auto t, auto ac) {
        using T = typename decltype(t)::type;
        constexpr int ACT = decltype(ac)::value;
        const GemmPlainKernel kern = pl.fl ? expert_gemm_plain_kernel<T, ACT, true> : expert_gemm_plain_kernel<T, ACT, false>;
        return launch_lds(kern, (unsigned)pl.grid, pl.threads, (size_t)pl.lds_bytes, st, p, pl.entry);
      },
      [&] { tutel_set_error("%s: unknown activation %d", pl.entry, act); return -1; });
}
