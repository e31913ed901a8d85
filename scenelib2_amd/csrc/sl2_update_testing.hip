// TEST build only (libscenelib2_amd_test.so, -DSL2_TESTING): the superseded kernel variants of the dense EKF update with their
// launchers, and the update's test / calibration entry points - a translation unit of its own, linked into the TEST library
// alone.  launch_update (sl2_ekf_update.hip, its -DSL2_TESTING build) calls the launchers where the plan names their form; see
// include/scenelib2_amd_testing.h and scripts/variants.sh for what selects these kernels.
#include "sl2_update_dev.hpp"
#include "sl2_chol_diag.hpp"
#include "../../include/scenelib2_amd_testing.h"

namespace sl2 {

// ---------------------------------------------------------------------------
// k_build_A: At[a][i] = (P H^T)[i][a], a = 2j+r for the j-th successful feature.
// Column ld-1 carries the innovation nu (so that L^-1 nu and W nu fall out of the
// same substitution / SYRK).  Rows of padding up to a multiple of 32 are zeroed.
// One workgroup per sequence; a thread keeps the 7 pose entries of its column in
// registers and loops over the features (3 coalesced row reads of P + 2 coalesced row
// writes of At per feature, each a full contiguous row for the workgroup).
// (Maps beyond what k_build_AS takes are not built by the product - sl2_create rejects them: SL2_BUILD_VARIANT=0.)
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(512) k_build_A(const double* __restrict__ P, const double* __restrict__ f_Hx,
                                                 const double* __restrict__ f_Hy, const double* __restrict__ f_nu,
                                                 const int* __restrict__ succ_idx, const int* __restrict__ m_count,
                                                 double* __restrict__ At, int N, int ld, int mld) {
  // one workgroup per sequence; a thread owns column(s) i and loops over the features, so every
  // row of P / At is streamed as one contiguous burst by the workgroup
  const int b = blockIdx.x;
  const int cnt = m_count[b];
  if (cnt == 0) return;
  const int cnt_pad = (cnt + 15) / 16 * 16;
  double* Ab = At + (size_t)b * mld * ld;
  const double* Pb = P + (size_t)b * ld * ld;
  for (int i = threadIdx.x; i < ld; i += blockDim.x) {
    double pc[7];
#pragma unroll
    for (int c = 0; c < 7; ++c) pc[c] = (i < 13) ? Pb[(size_t)i * ld + c] : Pb[(size_t)c * ld + i];
#pragma unroll 4
    for (int j = 0; j < cnt; ++j) {
      const int f = succ_idx[(size_t)b * N + j];
      const size_t fi = (size_t)b * N + f;
      const int pos = 13 + 3 * f;
      double py[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) py[c] = Pb[(size_t)(pos + c) * ld + i];
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        double acc = 0.0;
#pragma unroll
        for (int c = 0; c < 7; ++c) acc += pc[c] * f_Hx[fi * 14 + r * 7 + c];
#pragma unroll
        for (int c = 0; c < 3; ++c) acc += py[c] * f_Hy[fi * 6 + r * 3 + c];
        if (i == ld - 1) acc = f_nu[fi * 2 + r];
        Ab[(size_t)(2 * j + r) * ld + i] = acc;
      }
    }
    for (int j = cnt; j < cnt_pad; ++j) {
      Ab[(size_t)(2 * j) * ld + i] = 0.0;
      Ab[(size_t)(2 * j + 1) * ld + i] = 0.0;
    }
  }
}

// ---------------------------------------------------------------------------
// k_build_S: S = H A + R, stored St[c][r] = S[r][c] (32x32 blocks on and below the block
// diagonal; the factorisation reads r >= c plus the full diagonal blocks).  Padding: identity.  A thread owns one row
// a of H (its 10 non-zeros in registers) and loops over 32 columns bb: per column
// 7 wave-uniform loads (pose part of At row bb) + 3 gathered loads within that row.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_build_S(const double* __restrict__ At, const double* __restrict__ f_Hx,
                                                 const double* __restrict__ f_Hy, const double* __restrict__ f_R,
                                                 const int* __restrict__ succ_idx, const int* __restrict__ m_count,
                                                 double* __restrict__ St, int N, int ld, int mld) {
  const int b = blockIdx.z;
  const int cnt = m_count[b];
  if (cnt == 0) return;
  const int mp = (2 * cnt + 31) / 32 * 32;
  const int a = blockIdx.y * 256 + threadIdx.x;
  const int bb0 = blockIdx.x * 32;
  if (a >= mp || bb0 >= mp) return;
  if (bb0 > (a | 31)) return;   // strictly above the block diagonal: never read by the factorisation
  double* Sb = St + (size_t)b * mld * mld;
  const int m = 2 * cnt;
  if (a >= m) {
    for (int bb = bb0; bb < bb0 + 32; ++bb) Sb[(size_t)bb * mld + a] = (a == bb) ? 1.0 : 0.0;
    return;
  }
  const int j = a >> 1, r = a & 1;
  const int fj = succ_idx[(size_t)b * N + j];
  const size_t fi = (size_t)b * N + fj;
  const int posj = 13 + 3 * fj;
  double hx[7], hy[3];
#pragma unroll
  for (int c = 0; c < 7; ++c) hx[c] = f_Hx[fi * 14 + r * 7 + c];
#pragma unroll
  for (int c = 0; c < 3; ++c) hy[c] = f_Hy[fi * 6 + r * 3 + c];
  const double Rn = f_R[fi];
  const double* Ab = At + (size_t)b * mld * ld;
#pragma unroll 4
  for (int bb = bb0; bb < bb0 + 32; ++bb) {
    double v;
    if (bb >= m) {
      v = 0.0;
    } else {
      const double* arow = Ab + (size_t)bb * ld;
      double acc = 0.0;
#pragma unroll
      for (int c = 0; c < 7; ++c) acc += hx[c] * arow[c];
#pragma unroll
      for (int c = 0; c < 3; ++c) acc += hy[c] * arow[posj + c];
      if (a == bb) acc += Rn;
      v = acc;
    }
    Sb[(size_t)bb * mld + a] = v;
  }
}

// ---------------------------------------------------------------------------
// Blocked Cholesky of S (right-looking over 32x32 blocks, three launches per
// block column J): diag -> panel -> trailing update.
// ---------------------------------------------------------------------------

__device__ __forceinline__ double fast_rcp(double p) {
  double r = __builtin_amdgcn_rcp(p);
  r = __builtin_fma(__builtin_fma(-p, r, 1.0), r, r);
  r = __builtin_fma(__builtin_fma(-p, r, 1.0), r, r);
  return r;
}
__device__ __forceinline__ double fast_rsqrt(double p) {
  double y = __builtin_amdgcn_rsq(p);
  y = y * __builtin_fma(-0.5 * p * y, y, 1.5);
  y = y * __builtin_fma(-0.5 * p * y, y, 1.5);
  return y;
}

// k_chol_diag: one wave per sequence factors the (already updated) 32x32 diagonal
// block entirely in registers: lane r holds row r; pivots and column entries are
// broadcast with v_readlane (scalar operands of the FP64 FMAs), so there is no LDS
// round trip in the 32-step dependency chain.  Then the triangle is inverted row-wise
// (lane k solves X[k][:] L = e_k) and both L_JJ (in place) and LinvT are written
// with coalesced stores.
// (Measured alternatives on MI355X, per launch at batch 1024: LDS-resident block with one
// row per lane 67 us; column broadcast through LDS 43 us; 256-thread cooperative version with
// two barriers per column 36 us; single wave, element-parallel in LDS 47 us; this one 35 us —
// every variant is bound by the ~1 us dependent chain per column, not by throughput.)
__global__ void __launch_bounds__(64) k_chol_diag(double* __restrict__ St, double* __restrict__ LinvT,
                                                  const int* __restrict__ m_count, int mld, int nblk_max, int J) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int cnt = m_count[b];
  if (cnt == 0) return;
  const int nblk = (2 * cnt + 31) / 32;
  if (J >= nblk) return;
  double* Sb = St + (size_t)b * mld * mld;
  const int o = J * 32;
  const int r = lane & 31;                    // lanes 32..63 mirror lanes 0..31 (results discarded)
  double a[32];
#pragma unroll
  for (int c = 0; c < 32; ++c) a[c] = Sb[(size_t)(o + c) * mld + o + r];   // a[c] = S[o+r][o+c]
#pragma unroll
  for (int c = 0; c < 32; ++c) {
    const double piv = readlane_f64(a[c], c);
    const double dinv = fast_rsqrt(piv);
    const double d = piv * dinv;
    const double l = (r == c) ? d : a[c] * dinv;
    a[c] = (r >= c) ? l : 0.0;
#pragma unroll
    for (int cc = c + 1; cc < 32; ++cc) {
      const double lcc = readlane_f64(a[c], cc);   // L[cc][c]
      a[cc] -= l * lcc;                            // meaningful for r >= cc
    }
  }
  // inverse, row-wise: lane k holds x[p] = Linv[k][p]
  double diag = 1.0;
#pragma unroll
  for (int c = 0; c < 32; ++c) diag = (r == c) ? a[c] : diag;   // static indexing only (no scratch)
  const double rinv = fast_rcp(diag);              // 1 / L[r][r]
  double x[32];
#pragma unroll
  for (int p = 31; p >= 0; --p) {
    double sacc = (r == p) ? 1.0 : 0.0;
#pragma unroll
    for (int i = p + 1; i < 32; ++i) sacc -= x[i] * readlane_f64(a[p], i);   // X[k][i] * L[i][p]
    x[p] = sacc * readlane_f64(rinv, p);
  }
  if (lane < 32) {
    double* Lb = LinvT + ((size_t)b * nblk_max + J) * 1024;
#pragma unroll
    for (int c = 0; c < 32; ++c) {
      Sb[(size_t)(o + c) * mld + o + r] = a[c];    // L[r][c] (zero above the diagonal)
      Lb[c * 32 + r] = x[c];                       // LinvT[p = c][k = r] = Linv[r][c]
    }
  }
}

// k_chol_panel: L[I][J] = S[I][J] * L_JJ^-T for every block row I > J; one wave
// per 32x32 tile.  In k-major storage: new[k][i] = sum_p Linv[k][p] * St[J+p][I+i].
__global__ void __launch_bounds__(64) k_chol_panel(double* __restrict__ St, const double* __restrict__ LinvT,
                                                   const int* __restrict__ m_count, int mld, int nblk_max, int J) {
  const int b = blockIdx.y, lane = threadIdx.x;
  const int cnt = m_count[b];
  if (cnt == 0) return;
  const int nblk = (2 * cnt + 31) / 32;
  const int I = J + 1 + blockIdx.x;
  if (I >= nblk) return;
  const int lo = lane & 15, hi = lane >> 4;
  double* Sb = St + (size_t)b * mld * mld;
  const double* Lb = LinvT + ((size_t)b * nblk_max + J) * 1024;
  v4d acc[2][2];
  for (int kt = 0; kt < 2; ++kt) for (int it = 0; it < 2; ++it) acc[kt][it] = (v4d){0, 0, 0, 0};
#pragma unroll
  for (int s = 0; s < 8; ++s) {
    const int p = 4 * s + hi;
    const double a0 = Lb[p * 32 + lo], a1 = Lb[p * 32 + 16 + lo];
    const double b0 = Sb[(size_t)(J * 32 + p) * mld + I * 32 + lo];
    const double b1 = Sb[(size_t)(J * 32 + p) * mld + I * 32 + 16 + lo];
    acc[0][0] = mfma_f64(a0, b0, acc[0][0]);
    acc[0][1] = mfma_f64(a0, b1, acc[0][1]);
    acc[1][0] = mfma_f64(a1, b0, acc[1][0]);
    acc[1][1] = mfma_f64(a1, b1, acc[1][1]);
  }
#pragma unroll
  for (int kt = 0; kt < 2; ++kt)
#pragma unroll
    for (int it = 0; it < 2; ++it)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        Sb[(size_t)(J * 32 + 16 * kt + hi + 4 * r) * mld + I * 32 + 16 * it + lo] = acc[kt][it][r];
}

// k_chol_trail: S[I][K] -= L[I][J] L[K][J]^T for J < K <= I; one wave per tile.
__global__ void __launch_bounds__(64) k_chol_trail(double* __restrict__ St, const int* __restrict__ m_count, int mld, int J) {
  const int b = blockIdx.y, lane = threadIdx.x;
  const int cnt = m_count[b];
  if (cnt == 0) return;
  const int nblk = (2 * cnt + 31) / 32;
  // tile index -> (I, K), lower triangle of the trailing matrix, row-major
  int t = blockIdx.x, ri = 0;
  while (t > ri) { t -= ri + 1; ++ri; }
  const int I = J + 1 + ri, K = J + 1 + t;
  if (I >= nblk) return;
  const int lo = lane & 15, hi = lane >> 4;
  double* Sb = St + (size_t)b * mld * mld;
  v4d acc[2][2];
#pragma unroll
  for (int jt = 0; jt < 2; ++jt)
#pragma unroll
    for (int it = 0; it < 2; ++it)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        acc[jt][it][r] = Sb[(size_t)(K * 32 + 16 * jt + hi + 4 * r) * mld + I * 32 + 16 * it + lo];
#pragma unroll
  for (int s = 0; s < 8; ++s) {
    const size_t row = (size_t)(J * 32 + 4 * s + hi) * mld;
    const double a0 = -Sb[row + K * 32 + lo], a1 = -Sb[row + K * 32 + 16 + lo];
    const double b0 = Sb[row + I * 32 + lo], b1 = Sb[row + I * 32 + 16 + lo];
    acc[0][0] = mfma_f64(a0, b0, acc[0][0]);
    acc[0][1] = mfma_f64(a0, b1, acc[0][1]);
    acc[1][0] = mfma_f64(a1, b0, acc[1][0]);
    acc[1][1] = mfma_f64(a1, b1, acc[1][1]);
  }
#pragma unroll
  for (int jt = 0; jt < 2; ++jt)
#pragma unroll
    for (int it = 0; it < 2; ++it)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        Sb[(size_t)(K * 32 + 16 * jt + hi + 4 * r) * mld + I * 32 + 16 * it + lo] = acc[jt][it][r];
}

// ---------------------------------------------------------------------------
// k_fwdsub: Vt = L^-1 At by blocked forward substitution.  Columns are
// independent: each wave owns 16 columns and walks the block rows J in order,
//   acc = At[J] - sum_{K<J} L[J][K] Vt[K] ;  Vt[J] = L_JJ^-1 acc.
// A lane re-reads only Vt elements it stored itself (D fragment == B fragment).
// The chain is latency-bound (every k-step needs 3 L2-resident operands); what hides
// it is occupancy (64 VGPRs -> 7 waves per SIMD) plus the unrolled k-loop, which puts
// 8 k-steps of loads in flight ahead of their MFMAs.  A last block whose upper 16
// rows are all padding skips them.  32 columns per wave give four independent
// accumulator chains and 4 MFMAs per 3 fragment loads.
// (Tried and measured slower on MI355X, batch 1024: L blocks through LDS with a 4-wave
// barrier per block, 0.72 ms; V^T resident in LDS with one wave per workgroup, 2.1 ms;
// an explicit two-stage register pipeline, 1.04 ms at 256 VGPRs — each loses the
// occupancy that hides the chain's latency.  This version: see profiles/.)
// ---------------------------------------------------------------------------
template <bool HALF>
__device__ __forceinline__ void fwd_kloop(v4d acc[2][2], const double* __restrict__ lrow, const double* vrow, int mld, int ld,
                                          int kend) {
#pragma unroll 4
  for (int kk = 0; kk < kend; kk += 4) {
    const double a0 = -lrow[(size_t)kk * mld];
    const double b0 = vrow[(size_t)kk * ld], b1 = vrow[(size_t)kk * ld + 16];
    acc[0][0] = mfma_f64(a0, b0, acc[0][0]);
    acc[0][1] = mfma_f64(a0, b1, acc[0][1]);
    if (!HALF) {
      const double a1 = -lrow[(size_t)kk * mld + 16];
      acc[1][0] = mfma_f64(a1, b0, acc[1][0]);
      acc[1][1] = mfma_f64(a1, b1, acc[1][1]);
    }
  }
}

// 2 waves per workgroup, 32 columns per wave (four independent accumulator chains per wave).
__global__ void __launch_bounds__(128) k_fwdsub(const double* __restrict__ At, double* Vt, const double* __restrict__ St,
                                                const double* __restrict__ LinvT, const int* __restrict__ m_count, int ld,
                                                int mld, int nblk_max, int B) {
  int b, ct;
  if (!xcd_map(ld / 64, B, &b, &ct)) return;
  const int cnt = m_count[b];
  if (cnt == 0) return;
  const int m = 2 * cnt;
  const int nblk = (m + 31) / 32;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lo = lane & 15, hi = lane >> 4;
  const int i0 = ct * 64 + wave * 32;
  const double* Ab = At + (size_t)b * mld * ld;
  double* Vb = Vt + (size_t)b * mld * ld;
  const double* Sb = St + (size_t)b * mld * mld;
  for (int J = 0; J < nblk; ++J) {
    const bool half = (J * 32 + 16 >= m);    // rows J*32+16.. are padding: skip the second row tile
    v4d acc[2][2];
#pragma unroll
    for (int jt = 0; jt < 2; ++jt)
#pragma unroll
      for (int it = 0; it < 2; ++it)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          acc[jt][it][r] = (jt == 1 && half) ? 0.0 : Ab[(size_t)(J * 32 + 16 * jt + hi + 4 * r) * ld + i0 + 16 * it + lo];
    const double* lrow = Sb + (size_t)hi * mld + J * 32 + lo;     // L[J*32 + lo (+16)][k], k = hi + 4 s
    const double* vrow = Vb + (size_t)hi * ld + i0 + lo;
    if (half) fwd_kloop<true>(acc, lrow, vrow, mld, ld, J * 32);
    else fwd_kloop<false>(acc, lrow, vrow, mld, ld, J * 32);
    const double* Lb = LinvT + ((size_t)b * nblk_max + J) * 1024;
    v4d out[2][2];
#pragma unroll
    for (int jt = 0; jt < 2; ++jt) for (int it = 0; it < 2; ++it) out[jt][it] = (v4d){0, 0, 0, 0};
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      const int p = 4 * s + hi;
      const double a0 = Lb[p * 32 + lo];
      const double b0 = acc[s >> 2][0][s & 3], b1 = acc[s >> 2][1][s & 3];
      out[0][0] = mfma_f64(a0, b0, out[0][0]);
      out[0][1] = mfma_f64(a0, b1, out[0][1]);
      if (!half) {
        const double a1 = Lb[p * 32 + 16 + lo];
        out[1][0] = mfma_f64(a1, b0, out[1][0]);
        out[1][1] = mfma_f64(a1, b1, out[1][1]);
      }
    }
#pragma unroll
    for (int jt = 0; jt < 2; ++jt) {
      if (jt == 1 && half) continue;
#pragma unroll
      for (int it = 0; it < 2; ++it)
#pragma unroll
        for (int r = 0; r < 4; ++r) Vb[(size_t)(J * 32 + 16 * jt + hi + 4 * r) * ld + i0 + 16 * it + lo] = out[jt][it][r];
    }
  }
}

// ---------------------------------------------------------------------------
// The launchers of the superseded kernels above: launch_update calls them where the plan (sl2_update_plan.hpp, with
// UpdateShape::superseded) names their form - BuildForm::kTwoPass, CholForm::kPerBlock, FwdForm::kReread.
// ---------------------------------------------------------------------------
int launch_build_two_pass(sl2_engine* e, int threads) {
  const int B = e->B;
  {
    LaunchScope ls(e, "k_build_A", true);
    hipLaunchKernelGGL(k_build_A, dim3(B), dim3(threads), 0, e->stream, e->P, e->f_Hx, e->f_Hy, e->f_nu, e->succ_idx,
                       e->m_gate, e->At, e->N, e->ld, e->mld);
    SL2_HIP(hipGetLastError());
  }
  {
    LaunchScope ls(e, "k_build_S");
    dim3 grid(e->mld / 32, (e->mld + 255) / 256, B);
    hipLaunchKernelGGL(k_build_S, grid, dim3(256), 0, e->stream, e->At, e->f_Hx, e->f_Hy, e->f_R, e->succ_idx, e->m_gate,
                       e->St, e->N, e->ld, e->mld);
    SL2_HIP(hipGetLastError());
  }
  return SL2_OK;
}

// three launches per block column
int launch_chol_per_block(sl2_engine* e) {
  const int B = e->B;
  for (int J = 0; J < e->nblk_max; ++J) {
    {
      LaunchScope ls(e, "k_chol_diag");
      hipLaunchKernelGGL(k_chol_diag, dim3(B), dim3(64), 0, e->stream, e->St, e->LinvT, e->m_gate, e->mld, e->nblk_max, J);
      SL2_HIP(hipGetLastError());
    }
    const int rem = e->nblk_max - 1 - J;
    if (rem > 0) {
      {
        LaunchScope ls(e, "k_chol_panel");
        hipLaunchKernelGGL(k_chol_panel, dim3(rem, B), dim3(64), 0, e->stream, e->St, e->LinvT, e->m_gate, e->mld,
                           e->nblk_max, J);
        SL2_HIP(hipGetLastError());
      }
      {
        LaunchScope ls(e, "k_chol_trail");
        hipLaunchKernelGGL(k_chol_trail, dim3(rem * (rem + 1) / 2, B), dim3(64), 0, e->stream, e->St, e->m_gate, e->mld, J);
        SL2_HIP(hipGetLastError());
      }
    }
  }
  return SL2_OK;
}

int launch_fwdsub_reread(sl2_engine* e) {
  const int B = e->B;
  LaunchScope ls(e, "k_fwdsub", true);
  hipLaunchKernelGGL(k_fwdsub, dim3(xcd_grid(e->ld / 64, B)), dim3(128), 0, e->stream, e->At, e->Vt, e->St, e->LinvT,
                     e->m_gate, e->ld, e->mld, e->nblk_max, B);
  SL2_HIP(hipGetLastError());
  return SL2_OK;
}

// ---------------------------------------------------------------------------
// Debug GEMM on the same fragment conventions (tests the MFMA layout):
// C[m][n] = sum_k XT[k][m] YT[k][n], one wave per 32x32 tile.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(64) k_gemm_kt(const double* __restrict__ XT, int ldx, const double* __restrict__ YT, int ldy,
                                                int K, double* __restrict__ C, int ldc) {
  const int lane = threadIdx.x;
  const int lo = lane & 15, hi = lane >> 4;
  const int i0 = blockIdx.y * 32, j0 = blockIdx.x * 32;
  v4d acc[2][2];
  for (int it = 0; it < 2; ++it) for (int jt = 0; jt < 2; ++jt) acc[it][jt] = (v4d){0, 0, 0, 0};
  for (int k = 0; k < K; k += 4) {
    const double a0 = XT[(size_t)(k + hi) * ldx + i0 + lo], a1 = XT[(size_t)(k + hi) * ldx + i0 + 16 + lo];
    const double b0 = YT[(size_t)(k + hi) * ldy + j0 + lo], b1 = YT[(size_t)(k + hi) * ldy + j0 + 16 + lo];
    acc[0][0] = mfma_f64(a0, b0, acc[0][0]);
    acc[0][1] = mfma_f64(a0, b1, acc[0][1]);
    acc[1][0] = mfma_f64(a1, b0, acc[1][0]);
    acc[1][1] = mfma_f64(a1, b1, acc[1][1]);
  }
  for (int it = 0; it < 2; ++it)
    for (int jt = 0; jt < 2; ++jt)
      for (int r = 0; r < 4; ++r) C[(size_t)(i0 + 16 * it + hi + 4 * r) * ldc + j0 + 16 * jt + lo] = acc[it][jt][r];
}

}  // namespace sl2

extern "C" int sl2_debug_update_plan(sl2_engine* e, int group, int* out, int n) {
  using namespace sl2;
  if (!e || !out || group < 0 || group >= (int)e->root->groups.size() || n < kUpdatePlanInts) return SL2_ERR_INVALID;
  update_plan_ints(make_update_plan(update_shape(e->root->groups[group])), out);
  return SL2_OK;
}

extern "C" int sl2_debug_gemm_kt(int device, const double* XT, int ldx, const double* YT, int ldy, int M, int N, int K,
                                 double* C, int ldc) {
  using namespace sl2;
  if (!XT || !YT || !C || M % 32 || N % 32 || K % 4 || M <= 0 || N <= 0 || K <= 0) return SL2_ERR_INVALID;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { set_error("no HIP device"); return SL2_ERR_NO_DEVICE; }
  SL2_HIP(hipSetDevice(device));
  double *dX = nullptr, *dY = nullptr, *dC = nullptr;
  SL2_HIP(hipMalloc(&dX, sizeof(double) * (size_t)K * ldx));
  SL2_HIP(hipMalloc(&dY, sizeof(double) * (size_t)K * ldy));
  SL2_HIP(hipMalloc(&dC, sizeof(double) * (size_t)M * ldc));
  SL2_HIP(hipMemcpy(dX, XT, sizeof(double) * (size_t)K * ldx, hipMemcpyHostToDevice));
  SL2_HIP(hipMemcpy(dY, YT, sizeof(double) * (size_t)K * ldy, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_gemm_kt, dim3(N / 32, M / 32), dim3(64), 0, 0, dX, ldx, dY, ldy, K, dC, ldc);
  SL2_HIP(hipGetLastError());
  SL2_HIP(hipDeviceSynchronize());
  SL2_HIP(hipMemcpy(C, dC, sizeof(double) * (size_t)M * ldc, hipMemcpyDeviceToHost));
  hipFree(dX); hipFree(dY); hipFree(dC);
  return SL2_OK;
}

// ---------------------------------------------------------------------------
// Micro-benchmarks (debug ABI): the FP64 MFMA issue rate and a streaming copy,
// to confirm the peaks the roofline fractions are priced against.
// ---------------------------------------------------------------------------
namespace sl2 {
template <int NACC>
__global__ void __launch_bounds__(256) k_ubench_mfma(double* out, int iters) {
  v4d acc[NACC];
  for (int i = 0; i < NACC; ++i) acc[i] = (v4d){0, 0, 0, 0};
  double a = 1.0 + threadIdx.x * 1e-9, b = 1.0 - threadIdx.x * 1e-9;
  for (int it = 0; it < iters; ++it) {
#pragma unroll
    for (int i = 0; i < NACC; ++i) acc[i] = mfma_f64(a, b, acc[i]);
  }
  double s = 0;
  for (int i = 0; i < NACC; ++i) s += acc[i][0] + acc[i][1] + acc[i][2] + acc[i][3];
  if (s == 12345.678) out[0] = s;
}
__global__ void __launch_bounds__(256) k_ubench_copy(const double4* __restrict__ src, double4* __restrict__ dst, size_t n) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) dst[i] = src[i];
}
__global__ void __launch_bounds__(256) k_ubench_write(double4* __restrict__ dst, size_t n) {
  const double4 v = {1.0, 2.0, 3.0, 4.0};
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) dst[i] = v;
}
__global__ void __launch_bounds__(256) k_ubench_read(const double4* __restrict__ src, double* __restrict__ out, size_t n) {
  double s = 0;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const double4 v = src[i];
    s += v.x + v.y + v.z + v.w;
  }
  if (s == 12345.678) out[0] = s;
}
}  // namespace sl2

namespace sl2 {
__global__ void __launch_bounds__(256) k_ubench_fma64(double* out, int iters) {
  double acc[16];
  for (int i = 0; i < 16; ++i) acc[i] = threadIdx.x * 1e-9 + i;
  const double a = 1.0000001, b = 1e-9;
  for (int it = 0; it < iters; ++it) {
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = __builtin_fma(acc[i], a, b);
  }
  double s = 0;
  for (int i = 0; i < 16; ++i) s += acc[i];
  if (s == 12345.678) out[0] = s;
}
// half of the waves run the MFMA loop, the other half the VALU FMA loop: do the two pipes overlap?
__global__ void __launch_bounds__(256) k_ubench_mix(double* out, int iters) {
  const int wave = threadIdx.x >> 6;
  double s = 0;
  if (wave & 1) {
    double acc[16];
    for (int i = 0; i < 16; ++i) acc[i] = threadIdx.x * 1e-9 + i;
    const double a = 1.0000001, b = 1e-9;
    for (int it = 0; it < iters; ++it) {
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[i] = __builtin_fma(acc[i], a, b);
    }
    for (int i = 0; i < 16; ++i) s += acc[i];
  } else {
    v4d acc[4];
    for (int i = 0; i < 4; ++i) acc[i] = (v4d){0, 0, 0, 0};
    double a = 1.0 + threadIdx.x * 1e-9, b = 1.0 - threadIdx.x * 1e-9;
    for (int it = 0; it < iters; ++it) {
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[i] = mfma_f64(a, b, acc[i]);
    }
    for (int i = 0; i < 4; ++i) s += acc[i][0] + acc[i][1] + acc[i][2] + acc[i][3];
  }
  if (s == 12345.678) out[0] = s;
}
}  // namespace sl2

// which: 0 = FP64 MFMA TFLOP/s with 4 independent accumulators per wave, 2 blocks of 4 waves per CU
//        1 = same with 1 accumulator (dependent chain), 2 = streaming copy GB/s (read+write bytes),
//        3 = 8 accumulators, 4 blocks per CU, 4 = FP64 VALU FMA TFLOP/s, 5 = MFMA + VALU mixed,
//        6 = streaming write GB/s, 7 = streaming read GB/s
extern "C" int sl2_debug_microbench(int device, int which, double* result) {
  using namespace sl2;
  if (!result) return SL2_ERR_INVALID;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { set_error("no HIP device"); return SL2_ERR_NO_DEVICE; }
  SL2_HIP(hipSetDevice(device));
  hipEvent_t e0, e1;
  SL2_HIP(hipEventCreate(&e0));
  SL2_HIP(hipEventCreate(&e1));
  float ms = 0.f;
  if (which == 5) {
    // mixed: per block 2 MFMA waves (4 acc x iters MFMAs) + 2 VALU waves (16 x iters FMAs per lane)
    double* d = nullptr;
    SL2_HIP(hipMalloc(&d, 64));
    const int iters = 100000, blocks = 1024;
    for (int rep = 0; rep < 2; ++rep) {
      SL2_HIP(hipEventRecord(e0, 0));
      hipLaunchKernelGGL(k_ubench_mix, dim3(blocks), dim3(256), 0, 0, d, iters);
      SL2_HIP(hipEventRecord(e1, 0));
      SL2_HIP(hipEventSynchronize(e1));
    }
    SL2_HIP(hipEventElapsedTime(&ms, e0, e1));
    const double mf = (double)blocks * 2.0 * iters * 4.0 * 2048.0, vf = (double)blocks * 128.0 * iters * 16.0 * 2.0;
    *result = (mf + vf) / (ms * 1e-3) / 1e12;
    hipFree(d);
  } else if (which == 0 || which == 1 || which == 3 || which == 4) {
    double* d = nullptr;
    SL2_HIP(hipMalloc(&d, 64));
    const int iters = 200000;
    const int blocks = (which == 3 || which == 4) ? 1024 : 512;
    for (int rep = 0; rep < 2; ++rep) {
      SL2_HIP(hipEventRecord(e0, 0));
      if (which == 0) hipLaunchKernelGGL(k_ubench_mfma<4>, dim3(blocks), dim3(256), 0, 0, d, iters);
      else if (which == 1) hipLaunchKernelGGL(k_ubench_mfma<1>, dim3(blocks), dim3(256), 0, 0, d, iters);
      else if (which == 3) hipLaunchKernelGGL(k_ubench_mfma<8>, dim3(blocks), dim3(256), 0, 0, d, iters);
      else hipLaunchKernelGGL(k_ubench_fma64, dim3(blocks), dim3(256), 0, 0, d, iters);
      SL2_HIP(hipEventRecord(e1, 0));
      SL2_HIP(hipEventSynchronize(e1));
    }
    SL2_HIP(hipEventElapsedTime(&ms, e0, e1));
    if (which == 4) *result = (double)blocks * 256.0 * iters * 16.0 * 2.0 / (ms * 1e-3) / 1e12;
    else {
      const double nacc = which == 0 ? 4.0 : (which == 1 ? 1.0 : 8.0);
      *result = (double)blocks * 4.0 * iters * nacc * 2048.0 / (ms * 1e-3) / 1e12;
    }
    hipFree(d);
  } else {
    const size_t bytes = (size_t)1 << 30;
    double4 *s = nullptr, *t = nullptr;
    SL2_HIP(hipMalloc(&s, bytes));
    SL2_HIP(hipMalloc(&t, bytes));
    SL2_HIP(hipMemset(s, 1, bytes));
    for (int rep = 0; rep < 3; ++rep) {
      SL2_HIP(hipEventRecord(e0, 0));
      if (which == 6) hipLaunchKernelGGL(k_ubench_write, dim3(256 * 8), dim3(256), 0, 0, t, bytes / sizeof(double4));
      else if (which == 7) hipLaunchKernelGGL(k_ubench_read, dim3(256 * 8), dim3(256), 0, 0, s, (double*)t, bytes / sizeof(double4));
      else hipLaunchKernelGGL(k_ubench_copy, dim3(256 * 8), dim3(256), 0, 0, s, t, bytes / sizeof(double4));
      SL2_HIP(hipEventRecord(e1, 0));
      SL2_HIP(hipEventSynchronize(e1));
    }
    SL2_HIP(hipEventElapsedTime(&ms, e0, e1));
    *result = ((which == 6 || which == 7) ? 1.0 : 2.0) * bytes / (ms * 1e-3) / 1e9;
    hipFree(s); hipFree(t);
  }
  hipEventDestroy(e0); hipEventDestroy(e1);
  return SL2_OK;
}
