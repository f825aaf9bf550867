// Pieces shared by the skinny-M decode GEMMs (gemm_skinny.hip: bf16 weights,
// gemm_skinny_w8.hip: MX-fp8 weights): the 64x64 bf16 tile staging used for
// X (and for bf16 W), the K split, and the combine launches.  Both partials
// kernels write fp32 [SK, M, N]; the combine kernels are defined once in
// gemm_skinny.hip and carry every fused epilogue.
#pragma once
#include "common.h"

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8s;

__device__ __forceinline__ bf16x8s as_bf16x8s(s16x8 v) {
  union { s16x8 s; bf16x8s b; } u;
  u.s = v;
  return u.b;
}

// Stage a 64x64 bf16 tile (8 KiB) into linear LDS with read-side swizzle
// pre-applied to the global source.  2 x 16 B per thread.
__device__ __forceinline__ void stage64(const u16* __restrict__ g, size_t ld,
                                        u16* lds, int row0, int k0,
                                        int max_row) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const int e = (it * 256 + tid) * 8;
    const int row = e >> 6;
    const int wb = (e & 63) * 2;
    const int wsw = wb ^ ((row & 7) << 4);
    const u16* src = g + (size_t)min(row0 + row, max_row - 1) * ld + k0 + (wsw >> 1);
    u16* dst = lds + (size_t)(it * 256 + (tid & ~63)) * 8;
    __builtin_amdgcn_global_load_lds(
        (const __attribute__((address_space(1))) uint32_t*)src,
        (__attribute__((address_space(3))) uint32_t*)dst, 16, 0, 0);
  }
}

__device__ __forceinline__ s16x8 frag64(const u16* lds, int row, int byte) {
  return *reinterpret_cast<const s16x8*>(
      reinterpret_cast<const char*>(lds) + row * 128 + (byte ^ ((row & 7) << 4)));
}

// K split: Kc = K elements per split (multiple of 64); splits that would
// start at or past K are dropped from *SK.
static inline int af_skinny_split(int K, int* SK) {
  int Kc = ((K / *SK + 63) / 64) * 64;
  while ((*SK - 1) * Kc >= K) --*SK;  // drop empty splits
  return Kc;
}

__global__ void __launch_bounds__(256) gemm_skinny_combine_kernel(
    u16* __restrict__ out, u16* __restrict__ residual,
    const float* __restrict__ partial, int M, int N, int SK, int mode,
    const float* __restrict__ scale_ss, float inv_k, float eps);

__global__ void __launch_bounds__(256) gemm_skinny_combine_row_kernel(
    u16* __restrict__ out, u16* __restrict__ residual,
    const float* __restrict__ partial, float* __restrict__ ss_out,
    int M, int N, int SK);

// Fold partial [SK, M, N] into out with the epilogue selected by mode
// (0/1/2: combine_kernel, 4: combine_row_kernel).
static inline int af_skinny_combine(void* out, void* partial, void* residual,
                                    int M, int N, int K, int SK, int mode,
                                    const void* scale_ss, float eps,
                                    void* ss_out, hipStream_t st) {
  if (mode == 4) {
    if (N % 32) return 9007;
    dim3 g4(M, 8);
    gemm_skinny_combine_row_kernel<<<g4, 256, 0, st>>>(
        (u16*)out, (u16*)residual, (const float*)partial, (float*)ss_out,
        M, N, SK);
    return af_last_err();
  }
  const int cols = (mode == 2) ? N / 2 : N;
  i64 total = (i64)M * (cols / 4);
  int blocks = (int)((total + 255) / 256);
  if (blocks > 1024) blocks = 1024;
  gemm_skinny_combine_kernel<<<blocks, 256, 0, st>>>(
      (u16*)out, (u16*)residual, (const float*)partial, M, N, SK, mode,
      (const float*)scale_ss, 1.f / (float)K, eps);
  return af_last_err();
}
