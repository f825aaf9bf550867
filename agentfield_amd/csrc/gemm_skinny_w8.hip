// Skinny-M decode GEMM over MX-fp8 weights:  Y[M,N] = X[M,K] @ W[N,K]^T with
// W given as OCP e4m3fn bytes W8 [N,K] plus one E8M0 scale byte per
// 32-element K-block SW [N,K/32] (value 2^(b-127)), as quant.quantize_mx
// produces them.  The weight stream is N*K*(1 + 1/32) bytes, about half of
// the bf16 kernel's.
//
// An e4m3 value times a power of two is exactly representable in bf16, so
// the kernel rebuilds the bf16 weight in registers (cvt fp8->f32, multiply
// by the scale, keep the high 16 bits) and feeds the same bf16 MFMA as
// gemm_skinny_kernel, with the same K split, the same two
// mfma_f32_16x16x32_bf16 per 64 K in ascending K, the same B-fragment
// lane mapping and the same X staging.  Its fp32 partials are therefore
// bit-identical to gemm_skinny_kernel run on the dequantized bf16 matrix, and
// the shared combine kernels give bit-identical outputs in every mode.
//
// Domain: scale bytes 1..254 (b << 23 must be a normal fp32) and
// value * scale a normal fp32; e4m3fn's NaN codes 0x7f/0xff do not occur
// (quantize_mx clamps to +-448 and never emits them).  Codes 0x00/0x80 give
// +-0 under every scale because the scale is applied by multiplication.
#include "gemm_skinny.h"

// Stage a W8 tile [64 rows x 64 B] (4 KiB): one 16-byte global_load_lds per
// thread.  Thread t fills LDS bytes [16t, 16t+16) = row t>>2, physical
// 16-byte chunk t&3; the XOR swizzle is applied on the global source so that
// physical chunk p of row r holds logical chunk p ^ ((r>>2)&3).
__device__ __forceinline__ void stage_w8(const uint8_t* __restrict__ g,
                                         size_t ld, uint8_t* lds, int row0,
                                         int k0, int max_row) {
  const int tid = threadIdx.x;
  const int row = tid >> 2;
  const int chunk = (tid & 3) ^ ((row >> 2) & 3);
  const uint8_t* src =
      g + (size_t)min(row0 + row, max_row - 1) * ld + k0 + chunk * 16;
  uint8_t* dst = lds + (size_t)(tid & ~63) * 16;
  __builtin_amdgcn_global_load_lds(
      (const __attribute__((address_space(1))) uint32_t*)src,
      (__attribute__((address_space(3))) uint32_t*)dst, 16, 0, 0);
}

// The 8 weight bytes at logical byte offset `byte` (multiple of 8) of `row`.
// Why the ds_read_b64 is conflict-free: its banks are (addr/4) % 64 and
// lanes conflict within a 32-lane half, so a half must cover 32 distinct
// 8-byte units of the 256-B bank row.  With 64-B rows, rows r, r+4, r+8,
// r+12 share the same quarter of the bank row.  A half reads rows 0..15
// (lane&15) at two adjacent 8-byte units, i.e. one logical 16-byte chunk c;
// the four rows of a quarter differ in (r>>2)&3, so c ^ ((r>>2)&3) puts
// them on four different physical chunks: 4 rows x 2 units fill the
// quarter's 8 units exactly once.
__device__ __forceinline__ uint2 frag_w8(const uint8_t* lds, int row,
                                         int byte) {
  const int chunk = (byte >> 4) ^ ((row >> 2) & 3);
  return *reinterpret_cast<const uint2*>(lds + row * 64 + chunk * 16 +
                                         (byte & 8));
}

// The same for two adjacent sub-tiles at once: a W8 tile [64 rows x 128 B]
// (8 KiB), two 16-byte global_load_lds per thread.  Eight lanes fetch one
// whole 128-B line of a row, as the bf16 kernel's stage64 does; 64-B row
// segments cost the memory system as many requests as 128-B ones and the
// stream is bound by requests, not bytes.  Physical chunk p of row r holds
// logical chunk p ^ ((r>>1)&7).  A chunk past k1 (the split ends after the
// first sub-tile) is redirected to the last chunk inside the split: in
// bounds, and never read back.
__device__ __forceinline__ void stage_w8x2(const uint8_t* __restrict__ g,
                                           size_t ld, uint8_t* lds, int row0,
                                           int k, int k1, int max_row) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const int e = it * 256 + tid;
    const int row = e >> 3;
    const int chunk = (e & 7) ^ ((row >> 1) & 7);
    const uint8_t* src = g + (size_t)min(row0 + row, max_row - 1) * ld +
                         min(k + chunk * 16, k1 - 16);
    uint8_t* dst = lds + (size_t)(it * 256 + (tid & ~63)) * 16;
    __builtin_amdgcn_global_load_lds(
        (const __attribute__((address_space(1))) uint32_t*)src,
        (__attribute__((address_space(3))) uint32_t*)dst, 16, 0, 0);
  }
}

// Conflict-free by the same count with 128-B rows: rows r, r+2, ..., r+14
// share a half of the bank row and differ in (r>>1)&7, so one logical chunk
// lands on eight different physical chunks: 8 rows x 2 units fill the
// half's 16 units exactly once.
__device__ __forceinline__ uint2 frag_w8x2(const uint8_t* lds, int row,
                                           int byte) {
  const int chunk = (byte >> 4) ^ ((row >> 1) & 7);
  return *reinterpret_cast<const uint2*>(lds + row * 128 + chunk * 16 +
                                         (byte & 8));
}

// 8 e4m3 bytes (ascending k) x 2^(sb-127) -> 8 bf16, exact.
__device__ __forceinline__ bf16x8s dequant8(uint2 w, uint32_t sb) {
  union { uint32_t u; float f; } sc;
  sc.u = sb << 23;
  const f32x2 s = {sc.f, sc.f};
  union { f32x2 f; uint32_t u[2]; } p[4];
  p[0].f = __builtin_amdgcn_cvt_pk_f32_fp8((int)w.x, false) * s;
  p[1].f = __builtin_amdgcn_cvt_pk_f32_fp8((int)w.x, true) * s;
  p[2].f = __builtin_amdgcn_cvt_pk_f32_fp8((int)w.y, false) * s;
  p[3].f = __builtin_amdgcn_cvt_pk_f32_fp8((int)w.y, true) * s;
  // the products have at most 4 significant bits: the high half of the fp32
  // IS the bf16, whatever the rounding mode
  union { uint32_t u[4]; bf16x8s b; } o;
#pragma unroll
  for (int j = 0; j < 4; ++j)
    o.u[j] = __builtin_amdgcn_perm(p[j].u[1], p[j].u[0], 0x07060302u);
  return o.b;
}

// stage64 restricted to the first ROWS (multiple of 16, <= 64) rows of an X
// tile: same LDS image for those rows, so frag64 reads it unchanged; the
// rows no M tile uses are neither loaded nor given LDS.  A wave stages 8
// whole rows per pass, so the guard is wave-uniform.
template <int ROWS>
__device__ __forceinline__ void stage_x(const u16* __restrict__ g, size_t ld,
                                        u16* lds, int k0, int max_row) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    if (it * 32 + (tid >> 6) * 8 >= ROWS) continue;
    const int e = (it * 256 + tid) * 8;
    const int row = e >> 6;
    const int wb = (e & 63) * 2;
    const int wsw = wb ^ ((row & 7) << 4);
    const u16* src = g + (size_t)min(row, max_row - 1) * ld + k0 + (wsw >> 1);
    u16* dst = lds + (size_t)(it * 256 + (tid & ~63)) * 8;
    __builtin_amdgcn_global_load_lds(
        (const __attribute__((address_space(1))) uint32_t*)src,
        (__attribute__((address_space(3))) uint32_t*)dst, 16, 0, 0);
  }
}

// MT = number of 16-row M tiles (ceil(M/16)); grid (N/64, SK), block 256.
// KS = 64-K sub-tiles staged per pipeline step: where LDS allows (>= 4
// blocks per CU, the occupancy choose_sk's grid asks for) a step takes two,
// so that W8 is fetched in whole 128-B lines (stage_w8x2) and a split has
// half the barriers.  Sub-tiles are consumed in ascending K into the same
// accumulators, so the sum order (and every bit of the result) is that of
// 64-K steps.  Kc is a multiple of 64 only: the last step of a split may
// hold a single sub-tile.
template <int MT, int KS>
__global__ void __launch_bounds__(256) gemm_skinny_w8_kernel(
    float* __restrict__ partial, const u16* __restrict__ X,
    const uint8_t* __restrict__ W8, const uint8_t* __restrict__ SW, int M,
    int N, int K, int Kc) {
  constexpr int XBLKS = (MT + 3) / 4;  // 64-row stage blocks for X
  __shared__ __attribute__((aligned(16))) uint8_t sW[2][KS * 64 * 64];
  constexpr int XROWS = MT <= 4 ? MT * 16 : XBLKS * 64;  // X rows in LDS
  __shared__ u16 sX[2][KS][XROWS * 64];
  const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int nblk = blockIdx.x * 64;
  const int sk = blockIdx.y;
  const int k0 = sk * Kc;
  const int k1 = min(K, k0 + Kc);
  const int wrow = wid * 16 + (lane & 15);  // this lane's W row in the tile

  f32x4 acc[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) acc[mt] = f32x4{0, 0, 0, 0};

  // The lane's row has one scale byte per MFMA (32 K): the two bytes of a
  // 64-K sub-tile are one aligned 16-bit load (K/32 is even), fetched
  // straight from global one step ahead.
  const u16* srow = reinterpret_cast<const u16*>(
      SW + (size_t)(nblk + wrow) * (K >> 5));

  // stage the sub-tiles of the step starting at k (those inside the split)
  // into buffer `buf` and fetch their scales
  auto stage = [&](int buf, int k, uint32_t* sc) {
    if constexpr (KS == 2) stage_w8x2(W8, K, sW[buf], nblk, k, k1, N);
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      const int ks = k + s * 64;
      sc[s] = 0;
      if (KS == 1 || ks < k1) {
        if constexpr (KS == 1) stage_w8(W8, K, sW[buf], nblk, ks, N);
        if constexpr (MT <= 4) {
          stage_x<XROWS>(X, K, sX[buf][s], ks, M);
        } else {
#pragma unroll
          for (int xb = 0; xb < XBLKS; ++xb)
            stage64(X + (size_t)(xb * 64) * K, K, sX[buf][s] + xb * 64 * 64,
                    0, ks, M - xb * 64);
        }
        sc[s] = srow[ks >> 6];
      }
    }
  };

  int cur = 0;
  uint32_t sc[KS], sc_next[KS] = {};
  stage(0, k0, sc);
  __syncthreads();
  for (int k = k0; k < k1; k += 64 * KS) {
    if (k + 64 * KS < k1) stage(cur ^ 1, k + 64 * KS, sc_next);
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      if (KS == 1 || k + s * 64 < k1) {
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
          const int kel = kk * 32 + (lane >> 4) * 8;  // = byte offset in W8 row
          const uint2 wb = KS == 2
                               ? frag_w8x2(sW[cur], wrow, s * 64 + kel)
                               : frag_w8(sW[cur], wrow, kel);
          const bf16x8s bf = dequant8(wb, (sc[s] >> (8 * kk)) & 0xffu);
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) {
            const s16x8 af =
                frag64(sX[cur][s], mt * 16 + (lane & 15), kel * 2);
            acc[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                as_bf16x8s(af), bf, acc[mt], 0, 0, 0);
          }
        }
      }
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < KS; ++s) sc[s] = sc_next[s];
    cur ^= 1;
  }

  // C layout: lane l reg r -> C[m=(l>>4)*4+r][n=l&15]
  float* pbase = partial + (size_t)sk * M * N;
  const int ncol = nblk + wrow;
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const int mrow = mt * 16 + (lane >> 4) * 4;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      if (mrow + r < M)
        pbase[(size_t)(mrow + r) * N + ncol] = acc[mt][r];
    }
  }
}

AF_EXPORT int af_gemm_skinny_w8(void* out, void* partial, void* residual,
                                const void* X, const void* W8, const void* SW,
                                int M, int N, int K, int SK, int mode,
                                const void* scale_ss, float eps, void* ss_out,
                                void* stream) {
  if (M < 1 || M > 256) return 9005;
  if (N % 64 || K % 64) return 9006;
  hipStream_t st = (hipStream_t)stream;
  const int Kc = af_skinny_split(K, &SK);
  dim3 grid(N / 64, SK), blk(256);
  const int MT = (M + 15) / 16;
  // two sub-tiles per step while that keeps LDS <= 40 KiB (M <= 48)
#define AF_SK8_LAUNCH(MTV)                                                     \
  gemm_skinny_w8_kernel<MTV, (MTV <= 3 ? 2 : 1)><<<grid, blk, 0, st>>>(        \
      (float*)partial, (const u16*)X, (const uint8_t*)W8, (const uint8_t*)SW,  \
      M, N, K, Kc)
  switch (MT) {
    case 1: AF_SK8_LAUNCH(1); break;
    case 2: AF_SK8_LAUNCH(2); break;
    case 3: AF_SK8_LAUNCH(3); break;
    case 4: AF_SK8_LAUNCH(4); break;
    case 5: AF_SK8_LAUNCH(5); break;
    case 6: AF_SK8_LAUNCH(6); break;
    case 7: AF_SK8_LAUNCH(7); break;
    case 8: AF_SK8_LAUNCH(8); break;
    case 9: AF_SK8_LAUNCH(9); break;
    case 10: AF_SK8_LAUNCH(10); break;
    case 11: AF_SK8_LAUNCH(11); break;
    case 12: AF_SK8_LAUNCH(12); break;
    case 13: AF_SK8_LAUNCH(13); break;
    case 14: AF_SK8_LAUNCH(14); break;
    case 15: AF_SK8_LAUNCH(15); break;
    default: AF_SK8_LAUNCH(16); break;
  }
#undef AF_SK8_LAUNCH
  return af_skinny_combine(out, partial, residual, M, N, K, SK, mode,
                           scale_ss, eps, ss_out, st);
}
