// Skinny-M decode GEMM over MX-fp4 weights:  Y[M,N] = X[M,K] @ W[N,K]^T with
// W given as packed OCP e2m1 codes W4 [N,K/2] (element k in byte k>>1, even k
// in the low nibble; code = sign<<3 | exponent<<1 | mantissa, values 0, 1/2,
// 1, 3/2, 2, 3, 4, 6) plus one E8M0 scale byte per 32-element K-block
// SW [N,K/32] (value 2^(b-127)), as quant.quantize_mx4 produces them.  The
// weight stream is N*K*(1/2 + 1/32) bytes: just over half of the fp8 kernel's
// and about a quarter of the bf16 kernel's.
//
// An e2m1 value times a power of two is exactly representable in bf16, so the
// kernel rebuilds the bf16 weight in registers and feeds the same bf16 MFMA
// as gemm_skinny_kernel, with the same K split, the same two
// mfma_f32_16x16x32_bf16 per 64 K in ascending K, the same B-fragment lane
// mapping and the same X staging.  Its fp32 partials are therefore
// bit-identical to gemm_skinny_kernel run on the dequantized bf16 matrix, and
// the shared combine kernels give bit-identical outputs in every mode.
//
// Dequant: v_cvt_scalef32_pk_bf16_fp4 (byte `sel` of a dword x an fp32 scale
// -> two bf16), four per 8 elements, the scale built as b << 23.  Measured on
// MI355X with all 256 byte values in each byte position under scale bytes
// 1, 100, 127, 140 and 254: the low nibble of the selected byte is element
// 0, the high nibble element 1; the code table is the OCP one, the subnormal
// code 1 (+-1/2) included; codes 0 and 8 give +0 and -0 under every scale.
// That is the packing above with sel = byte index, so the builtin is used as
// it stands: no permutation, no table fallback.
//
// Weight path.  A 64-K sub-tile of W4 is 32 B per row, a quarter of a 128-B
// line, and the stream is bound by requests, not bytes (gemm_skinny_w8.hip).
// So W4 and X move at different cadences:
//   * W4 is staged in line tiles [64 rows x 128 B] = 256 K, aligned to 256 K,
//     into a ring of two; line L+1 is requested as soon as line L-1 has been
//     consumed, i.e. at the first step inside line L, and is then four 64-K
//     sub-steps ahead of its first use.
//   * X keeps the 64-K double buffer of the other skinny kernels (two
//     sub-tiles per step while LDS stays <= 40 KiB, as in the fp8 kernel), so
//     LDS does not grow with the 256-K W cadence.
// A split's k0 is a multiple of 64, not of 256: a split may begin and end
// inside a line.  Chunks of a line outside [k0, k1) are redirected to a chunk
// inside the split: in bounds, and never read back.
//
// Domain: M 1..256, N % 64 == 0, K % 64 == 0, scale bytes 1..254 (b << 23
// must be a normal fp32); every nibble code is legal.
#include "gemm_skinny.h"

typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2s;

// Stage the W4 line tile [64 rows x 128 B] whose first element is K index kl
// (multiple of 256): two 16-byte global_load_lds per thread, eight lanes per
// row fetch one whole line.  Thread e fills LDS bytes [16e, 16e+16) = row
// e>>3, physical chunk e&7; the XOR swizzle is applied on the global source
// so that physical chunk p of row r holds logical chunk p ^ ((r>>1)&7).  The
// source byte offset is clamped into the split [k0/2, k1/2 - 16].
__device__ __forceinline__ void stage_w4(const uint8_t* __restrict__ g,
                                         size_t ld, uint8_t* lds, int row0,
                                         int kl, int k0, int k1, int max_row) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const int e = it * 256 + tid;
    const int row = e >> 3;
    const int chunk = (e & 7) ^ ((row >> 1) & 7);
    const int off = min(max((kl >> 1) + chunk * 16, k0 >> 1), (k1 >> 1) - 16);
    const uint8_t* src = g + (size_t)min(row0 + row, max_row - 1) * ld + off;
    uint8_t* dst = lds + (size_t)(it * 256 + (tid & ~63)) * 16;
    __builtin_amdgcn_global_load_lds(
        (const __attribute__((address_space(1))) uint32_t*)src,
        (__attribute__((address_space(3))) uint32_t*)dst, 16, 0, 0);
  }
}

// The 4 weight bytes (8 codes) at logical byte offset `byte` (multiple of 4)
// of `row` in a line tile.  Why the ds_read_b32 is conflict-free: banks are
// (addr/4) % 64, so a 128-B row covers half of the 256-B bank row, rows of
// equal parity the same half.  One instruction reads rows 0..15 (lane&15) at
// the four adjacent dwords (lane>>4) of ONE logical 16-byte chunk c.  The
// eight rows of one parity differ in (r>>1)&7, so c ^ ((r>>1)&7) puts them on
// the eight different physical chunks of their half: 2 parities x 8 chunks x
// 4 dwords = 64 distinct banks for the 64 lanes, whether the hardware
// resolves conflicts per 32-lane half or over the whole wave.
__device__ __forceinline__ uint32_t frag_w4(const uint8_t* lds, int row,
                                            int byte) {
  const int chunk = (byte >> 4) ^ ((row >> 1) & 7);
  return *reinterpret_cast<const uint32_t*>(lds + row * 128 + chunk * 16 +
                                            (byte & 12));
}

// 8 e2m1 codes (ascending k: byte j holds elements 2j, 2j+1, low nibble
// first) x 2^(sb-127) -> 8 bf16, exact.
__device__ __forceinline__ bf16x8s dequant4(uint32_t w, uint32_t sb) {
  union { uint32_t u; float f; } sc;
  sc.u = sb << 23;
  union { bf16x2s p[4]; bf16x8s b; } o;
  o.p[0] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, sc.f, 0);
  o.p[1] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, sc.f, 1);
  o.p[2] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, sc.f, 2);
  o.p[3] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, sc.f, 3);
  return o.b;
}

// stage64's LDS image for the first ROWS (multiple of 16, <= 256) rows of X:
// row r at byte r*128, so frag64 reads it unchanged; rows no M tile uses are
// neither loaded nor given LDS.  A wave stages 8 whole rows per pass, so the
// guard is wave-uniform.
template <int ROWS>
__device__ __forceinline__ void stage_xrows(const u16* __restrict__ g,
                                            size_t ld, u16* lds, int k0,
                                            int max_row) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int it = 0; it < (ROWS + 31) / 32; ++it) {
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
// XS = 64-K X sub-tiles staged per pipeline step (one barrier per step).
// Sub-tiles are consumed in ascending K into the same accumulators, so the
// sum order (and every bit of the result) is that of 64-K steps.  Kc is a
// multiple of 64 only: the last step of a split may hold a single sub-tile,
// and with XS = 2 a step may straddle two W4 lines (both are resident: the
// ring holds the line of k and the one after it).
template <int MT, int XS>
__global__ void __launch_bounds__(256) gemm_skinny_w4_kernel(
    float* __restrict__ partial, const u16* __restrict__ X,
    const uint8_t* __restrict__ W4, const uint8_t* __restrict__ SW, int M,
    int N, int K, int Kc) {
  constexpr int XROWS = MT * 16;  // X rows in LDS
  __shared__ __attribute__((aligned(16))) uint8_t sW[2][64 * 128];
  __shared__ u16 sX[2][XS][XROWS * 64];
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

  // W4 ring: line kl lives in sW[(kl>>8)&1]; nl is the next line to request.
  // Line nl may overwrite line nl-512 once no step reads that one any more,
  // i.e. from the first step whose k lies in line nl-256 on.
  int nl = k0 & ~255;
  auto stage_line = [&](int upto) {
    if (nl < k1 && nl <= upto) {
      stage_w4(W4, (size_t)(K >> 1), sW[(nl >> 8) & 1], nblk, nl, k0, k1, N);
      nl += 256;
    }
  };
  // stage the X sub-tiles of the step starting at k (those inside the split)
  // into buffer `buf` and fetch their scales
  auto stage_x = [&](int buf, int k, uint32_t* sc) {
#pragma unroll
    for (int s = 0; s < XS; ++s) {
      const int ks = k + s * 64;
      sc[s] = 0;
      if (XS == 1 || ks < k1) {
        stage_xrows<XROWS>(X, K, sX[buf][s], ks, M);
        sc[s] = srow[ks >> 6];
      }
    }
  };

  int cur = 0;
  uint32_t sc[XS], sc_next[XS] = {};
  stage_line(k0);
  if constexpr (XS == 2) stage_line(k0 + 64);  // first step straddles
  stage_x(0, k0, sc);
  __syncthreads();
  for (int k = k0; k < k1; k += 64 * XS) {
    stage_line(k + 256);
    if (k + 64 * XS < k1) stage_x(cur ^ 1, k + 64 * XS, sc_next);
#pragma unroll
    for (int s = 0; s < XS; ++s) {
      const int ks = k + s * 64;
      if (XS == 1 || ks < k1) {
        const uint8_t* wl = sW[(ks >> 8) & 1];
        const int lb = (ks & 255) >> 1;  // byte offset of the sub-tile
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
          const int kel = kk * 32 + (lane >> 4) * 8;
          const uint32_t wb = frag_w4(wl, wrow, lb + (kel >> 1));
          const bf16x8s bf = dequant4(wb, (sc[s] >> (8 * kk)) & 0xffu);
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
    for (int s = 0; s < XS; ++s) sc[s] = sc_next[s];
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

AF_EXPORT int af_gemm_skinny_w4(void* out, void* partial, void* residual,
                                const void* X, const void* W4, const void* SW,
                                int M, int N, int K, int SK, int mode,
                                const void* scale_ss, float eps, void* ss_out,
                                void* stream) {
  if (M < 1 || M > 256) return 9005;
  if (N % 64 || K % 64) return 9006;
  hipStream_t st = (hipStream_t)stream;
  const int Kc = af_skinny_split(K, &SK);
  dim3 grid(N / 64, SK), blk(256);
  const int MT = (M + 15) / 16;
  // two X sub-tiles per step while that keeps LDS <= 40 KiB (M <= 48)
#define AF_SK4_LAUNCH(MTV)                                                     \
  gemm_skinny_w4_kernel<MTV, (MTV <= 3 ? 2 : 1)><<<grid, blk, 0, st>>>(        \
      (float*)partial, (const u16*)X, (const uint8_t*)W4, (const uint8_t*)SW,  \
      M, N, K, Kc)
  switch (MT) {
    case 1: AF_SK4_LAUNCH(1); break;
    case 2: AF_SK4_LAUNCH(2); break;
    case 3: AF_SK4_LAUNCH(3); break;
    case 4: AF_SK4_LAUNCH(4); break;
    case 5: AF_SK4_LAUNCH(5); break;
    case 6: AF_SK4_LAUNCH(6); break;
    case 7: AF_SK4_LAUNCH(7); break;
    case 8: AF_SK4_LAUNCH(8); break;
    case 9: AF_SK4_LAUNCH(9); break;
    case 10: AF_SK4_LAUNCH(10); break;
    case 11: AF_SK4_LAUNCH(11); break;
    case 12: AF_SK4_LAUNCH(12); break;
    case 13: AF_SK4_LAUNCH(13); break;
    case 14: AF_SK4_LAUNCH(14); break;
    case 15: AF_SK4_LAUNCH(15); break;
    default: AF_SK4_LAUNCH(16); break;
  }
#undef AF_SK4_LAUNCH
  return af_skinny_combine(out, partial, residual, M, N, K, SK, mode,
                           scale_ss, eps, ss_out, st);
}
