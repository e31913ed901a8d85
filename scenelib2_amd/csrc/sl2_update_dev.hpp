// Device helpers of the dense EKF update that more than one of its translation units uses (sl2_update_build.hip,
// sl2_update_chol.hip, sl2_update_fwdsub.hip, sl2_update_syrk.hip, sl2_update_testing.hip).  A helper with one user lives with
// that user.
#pragma once
#include "sl2_common.hpp"

namespace sl2 {

typedef double v4d __attribute__((ext_vector_type(4)));

__device__ __forceinline__ v4d mfma_f64(double a, double b, v4d c) {
  return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}

// Streaming accesses (the `nt` bit of global_load / global_store): for operands a kernel touches exactly once, beside the ones
// that are re-read (S / L, the V^T panels).  A hint only: no arithmetic and no ordering changes; what it gains is measured site
// by site (profiles/update_streams_ab.json: the bytes the counters see do not change, the time does).  Any pointer to double or to an ext_vector_type of 2 or 4 doubles (v4d; the HIP double2 / double4 structs are not
// accepted by the builtins), in any address space.  The policy per stream: DESIGN section 4.
template <class Ptr>
__device__ __forceinline__ auto load_stream(Ptr p) { return __builtin_nontemporal_load(p); }
template <class Ptr, class T>
__device__ __forceinline__ void store_stream(Ptr p, T v) { __builtin_nontemporal_store(v, p); }

constexpr int kSyrkKC = 16;       // K rows per chunk (k_syrk, k_fwd_gemm, k_chol_syrk)

// ---------------------------------------------------------------------------
// The K loop of k_syrk as a building block for the large-map GEMMs (k_fwd_gemm, k_chol_syrk): a 64x64 tile, four waves of
// 32x32, acc[it][jt][r] += sum_k A[k][wi + 16 it + 4 r + hi] * B[k][wj + 16 jt + lo] over `nchunk` chunks of 16 k-rows,
// both operands k-major in memory (row segments), staged through the 32 KB swapped-half-row LDS layout with the register
// prefetch two chunks ahead.  (Rounds 1-2 ran these two kernels on the first SYRK pipeline - 40 KB at pitch 80, one
// chunk ahead: 49.5 and 39 TFLOP/s at configs[4] against k_syrk's 59.)
// ---------------------------------------------------------------------------
__device__ __forceinline__ void kpanel_product(const double* __restrict__ A, size_t lda, const double* __restrict__ Bm, size_t ldb,
                                               int nchunk, bool idle, int wi, int wj, double (&sAB)[2][2][kSyrkKC * 64],
                                               v4d (&acc)[2][2]) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int lo = lane & 15, hi = lane >> 4;
  const int kr = tid >> 4, c2 = (tid & 15) * 2;
  const double* gA = A + (size_t)kr * lda + c2;
  const double* gB = Bm + (size_t)kr * ldb + c2;
  struct Stage { double2 a0, a1, b0, b1; };
  auto stage_load = [&](int chunk) {
    Stage r;
    r.a0 = *(const double2*)(gA + (size_t)chunk * kSyrkKC * lda); r.a1 = *(const double2*)(gA + (size_t)chunk * kSyrkKC * lda + 32);
    r.b0 = *(const double2*)(gB + (size_t)chunk * kSyrkKC * ldb); r.b1 = *(const double2*)(gB + (size_t)chunk * kSyrkKC * ldb + 32);
    return r;
  };
  auto stage_store = [&](int buf, const Stage& r) {
    const int cs = c2 ^ ((kr & 1) << 4);
    *(double2*)&sAB[buf][0][kr * 64 + cs] = r.a0;
    *(double2*)&sAB[buf][0][kr * 64 + 32 + cs] = r.a1;
    *(double2*)&sAB[buf][1][kr * 64 + cs] = r.b0;
    *(double2*)&sAB[buf][1][kr * 64 + 32 + cs] = r.b1;
  };
  auto chunk_mfma = [&](int buf) {
    const int sw = (hi & 1) << 4;
    const double* pa = &sAB[buf][0][hi * 64 + wi + lo];
    const double* pb = &sAB[buf][1][hi * 64 + wj + lo];
#pragma unroll
    for (int ks = 0; ks < kSyrkKC / 4; ++ks) {
      const double a0 = pa[ks * 256 + sw], a1 = pa[ks * 256 + (sw ^ 16)];
      const double b0 = pb[ks * 256 + sw], b1 = pb[ks * 256 + (sw ^ 16)];
      acc[0][0] = mfma_f64(a0, b0, acc[0][0]);
      acc[0][1] = mfma_f64(a0, b1, acc[0][1]);
      acc[1][0] = mfma_f64(a1, b0, acc[1][0]);
      acc[1][1] = mfma_f64(a1, b1, acc[1][1]);
    }
  };
  if (nchunk <= 0) return;
  Stage r0 = stage_load(0);
  Stage r1 = r0;
  if (nchunk > 1) r1 = stage_load(1);
  for (int ch = 0; ch < nchunk; ch += 2) {
    stage_store(0, r0);
    __syncthreads();
    if (ch + 2 < nchunk) r0 = stage_load(ch + 2);
    if (!idle) chunk_mfma(0);
    if (ch + 1 >= nchunk) break;
    stage_store(1, r1);
    __syncthreads();
    if (ch + 3 < nchunk) r1 = stage_load(ch + 3);
    if (!idle) chunk_mfma(1);
  }
}

}  // namespace sl2
