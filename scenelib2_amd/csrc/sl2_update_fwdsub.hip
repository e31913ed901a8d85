// EKF update, third phase: V = A L^-T by blocked forward substitution, and with the same kernel the panel solve of the
// panel-wise Cholesky (the algebra and the k-major storage: sl2_ekf_update.hip).
#include "sl2_update_dev.hpp"

namespace sl2 {

// ---------------------------------------------------------------------------
// k_fwdsub_lds<NB>: forward substitution with BOTH operands on chip.  A workgroup of four
// waves owns a 64-column tile of the state (16 columns per wave):
//   * the solved block rows of V^T stay in registers: the MFMA D fragment of block K is, unchanged,
//     the B fragment of every later product with it (NB = mld/32 block rows of a 16-column strip
//     = NB*16 VGPRs);
//   * the 32x32 tiles of L (and the inverted diagonal blocks) are streamed once per
//     workgroup through LDS, double-buffered: the global loads of tile t+1 fly under the
//     MFMAs of tile t, one barrier per tile (the scheme of k_syrk).
// Per k-step a wave issues two ds_read_b64 and two MFMAs and nothing else: no global load
// sits on the accumulator chain, which is what bounded k_fwdsub (sl2_update_testing.hip: every k-step there waits
// on three L2-resident operands).
// ---------------------------------------------------------------------------
constexpr int kFwdPitch = 48;   // LDS row pitch (doubles): the two k-rows read by a 32-lane group land on disjoint banks

template <int NB>
// (At, Vt and St are NOT __restrict__: the panel solve of the large-system Cholesky calls this kernel in place, with all three
// on the factor's own storage - every element is read by the lane that later overwrites it, before it does.)
__global__ void __launch_bounds__(256, (NB <= 8 ? 3 : 2)) k_fwdsub_lds(const double* At, double* Vt,
                                                    const double* St, const double* __restrict__ LinvT,
                                                    const int* __restrict__ m_count, int ld, int mld, int nblk_max, int B,
                                                    int J0, int col0, int ntile, int nb_cap) {
  // J0: first block row of this launch.  For maps of more than 13 blocks the substitution runs in groups of
  // NB = 8 block rows: k_fwd_gemm first subtracts the contribution of all earlier groups from the group's
  // rows of At, then this kernel solves within the group (block indices below are relative to J0).
  // col0 / ntile: the 64-column tiles col0 + 64 t, t < ntile, of the right-hand side (0, ld / 64 for the EKF substitution;
  // the panel solve of the large-system Cholesky passes the columns below its panel).  nb_cap caps the block rows solved.
  int b, ct;
  if (!xcd_map(ntile, B, &b, &ct)) return;
  const int cnt = m_count[b];
  if (cnt == 0) return;
  int m = 2 * cnt - 32 * J0;                // rows left from block J0 on
  if (m <= 0) return;
  if (m > 32 * nb_cap) m = 32 * nb_cap;
  const int nblk = (m + 31) / 32;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lo = lane & 15, hi = lane >> 4;
  const int i0 = col0 + ct * 64 + wave * 16;
  const double* Ab = At + (size_t)b * mld * ld + (size_t)J0 * 32 * ld;
  double* Vb = Vt + (size_t)b * mld * ld + (size_t)J0 * 32 * ld;
  const double* Sb = St + (size_t)b * mld * mld + (size_t)J0 * 32 * mld + J0 * 32;
  const double* Lb = LinvT + ((size_t)b * nblk_max + J0) * 1024;
  __shared__ double sL[2][32 * kFwdPitch];
  // staging role: row `srow` of the tile (contraction index), 4 consecutive doubles at column `sc4`.  (Lanes 0 and 4 of a
  // row's eight share their banks in the ds_write_b128: SQ_LDS_BANK_CONFLICT 8.6e6 per launch.  Round 4 tried the cure that
  // worked in k_syrk - two pieces of two doubles per thread, so that a store's eight lanes write 128 consecutive bytes - and
  // measured it SLOWER on the same box, 0.331 against 0.322-0.324 ms (profiles/r04_fwdsub_staging_ab.txt): twice the global
  // load instructions in front of every barrier cost more than the conflict cycles, which sit under the MFMAs here.)
  const int srow = tid >> 3, sc4 = (tid & 7) * 4;
  const int soff = srow * kFwdPitch + sc4;
  // tile (J, K): K < J -> L[J][K] from St (k-major), K == J -> LinvT block J
#define SL2_TILE_PTR(Jv, Kv) \
  (((Kv) < (Jv)) ? (Sb + (size_t)((Kv) * 32 + srow) * mld + (Jv) * 32 + sc4) : (Lb + (size_t)(Jv) * 1024 + srow * 32 + sc4))
  double4 pre = *(const double4*)SL2_TILE_PTR(0, 0);
  // In the EKF substitution At is read once and Vt is next read by another launch: both are streaming accesses (load_stream /
  // store_stream).  Measured at NB = 7, medians of five alternated processes (profiles/update_streams_ab.json): 0.306-0.314 ms
  // against 0.328 with plain accesses; the loads alone 0.323, the stores alone 0.325 - it takes both.  The panel solve runs in
  // place on the factor, which the following launches re-read, and must stay plain.  The kernel has one symbol per NB whoever
  // launches it (tests/test_update_units.py), so the instantiations launch_panel_solve names are plain for the EKF substitution
  // as well.  (A run-time choice between the two uses compiles to plain accesses; both bodies in one kernel cost <8> twenty more
  // spilled registers and <13> forty.)
  constexpr bool kStream = (NB != 8 && NB != kCholPanelBlocks);
  auto load_at = [](const double* p) { if constexpr (kStream) return load_stream(p); else return *p; };
  auto store_vt = [](double* p, double v) { if constexpr (kStream) store_stream(p, v); else *p = v; };
  v4d V[NB][2];
  v4d at[2];
  const bool half0 = (16 >= m);
#pragma unroll
  for (int jt = 0; jt < 2; ++jt)
#pragma unroll
    for (int r = 0; r < 4; ++r) at[jt][r] = (jt == 1 && half0) ? 0.0 : load_at(&Ab[(size_t)(16 * jt + hi + 4 * r) * ld + i0 + lo]);
  int t = 0;   // running tile counter (buffer parity)
#pragma unroll
  for (int J = 0; J < NB; ++J) {
    if (J < nblk) {
      const bool half = (J * 32 + 16 >= m);    // rows J*32+16.. are padding
      v4d acc[2];
      acc[0] = (v4d){0, 0, 0, 0};
      acc[1] = (v4d){0, 0, 0, 0};
      v4d rhs[2];
#pragma unroll
      for (int K = 0; K <= J; ++K) {
        double* buf = sL[t & 1];
        *(double4*)&buf[soff] = pre;
        __syncthreads();
        // next tile of the stream (uniform control flow: nblk is per sequence = per workgroup)
        if (K < J) pre = *(const double4*)SL2_TILE_PTR(J, K + 1);
        else if (J + 1 < nblk && J + 1 < NB) pre = *(const double4*)SL2_TILE_PTR(J + 1, 0);
        const double* pa = buf + hi * kFwdPitch + lo;
        if (K < J) {
#pragma unroll
          for (int s = 0; s < 8; ++s) {
            const double bv = V[K][s >> 2][s & 3];
            acc[0] = mfma_f64(pa[4 * s * kFwdPitch], bv, acc[0]);
            if (!half) acc[1] = mfma_f64(pa[4 * s * kFwdPitch + 16], bv, acc[1]);
          }
        } else {
          // rhs = At[J] - sum_K L[J][K] V[K];  V[J] = Linv_JJ rhs  (Linv lower triangular: rows 0..15 need p < 16 only)
#pragma unroll
          for (int jt = 0; jt < 2; ++jt) rhs[jt] = at[jt] - acc[jt];
          if (J + 1 < nblk && J + 1 < NB) {   // prefetch the next block row of At under the diagonal product
            const bool halfn = ((J + 1) * 32 + 16 >= m);
#pragma unroll
            for (int jt = 0; jt < 2; ++jt)
#pragma unroll
              for (int r = 0; r < 4; ++r)
                at[jt][r] = (jt == 1 && halfn) ? 0.0 : load_at(&Ab[(size_t)((J + 1) * 32 + 16 * jt + hi + 4 * r) * ld + i0 + lo]);
          }
          v4d out[2];
          out[0] = (v4d){0, 0, 0, 0};
          out[1] = (v4d){0, 0, 0, 0};
#pragma unroll
          for (int s = 0; s < 8; ++s) {
            const double bv = rhs[s >> 2][s & 3];
            if (s < 4) out[0] = mfma_f64(pa[4 * s * kFwdPitch], bv, out[0]);
            if (!half) out[1] = mfma_f64(pa[4 * s * kFwdPitch + 16], bv, out[1]);
          }
          V[J][0] = out[0];
          V[J][1] = out[1];
#pragma unroll
          for (int jt = 0; jt < 2; ++jt) {
            if (jt == 1 && half) continue;
#pragma unroll
            for (int r = 0; r < 4; ++r) store_vt(&Vb[(size_t)(J * 32 + 16 * jt + hi + 4 * r) * ld + i0 + lo], out[jt][r]);
          }
        }
        ++t;
      }
    }
  }
#undef SL2_TILE_PTR
}

// ---------------------------------------------------------------------------
// k_fwdsub_ksplit: the forward substitution for SMALL batches, where k_fwdsub_lds is a chain, not a throughput problem:
// there one wavefront walks all (J + 1) tile products of every block row of its 16 columns one after the other - 23
// dependent 16-MFMA steps, 26 us for a single sequence.  Here a four-wave workgroup owns ONE 16-column strip: the solved
// block rows live in LDS (the B fragments of every wave), the J products of block row J are dealt to the four waves,
// their partial sums meet in LDS, and wave 0 applies the inverted diagonal block.  Same sums in a different association
// (four partial sums): tolerance parity like every other variant.  Up to kKsMaxBlocks 32-blocks.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_fwdsub_ksplit(const double* __restrict__ At, double* __restrict__ Vt,
                                                       const double* __restrict__ St, const double* __restrict__ LinvT,
                                                       const int* __restrict__ m_count, int ld, int mld, int nblk_max, int B) {
  int b, ct;
  if (!xcd_map(ld / 16, B, &b, &ct)) return;
  const int cnt = m_count[b];
  if (cnt == 0) return;
  const int nblk = (2 * cnt + 31) / 32;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lo = lane & 15, hi = lane >> 4;
  const int i0 = ct * 16;
  const double* Ab = At + (size_t)b * mld * ld;
  double* Vb = Vt + (size_t)b * mld * ld;
  const double* Sb = St + (size_t)b * mld * mld;
  const double* Lb = LinvT + (size_t)b * nblk_max * 1024;
  __shared__ double sV[kKsMaxBlocks][32 * 16];      // solved block rows: [row][column]
  __shared__ double sPart[4][32 * 16];              // the waves' partial sums of the current block row
  // Operand prefetch (registers): the L tile of the wave's NEXT product - its (J, K) pairs are known in advance: K = wave,
  // wave + 4, ... < J for J = wave + 1, wave + 2, ... -, and for wave 0 the next block row of At and the inverted diagonal
  // block of the current one: nothing on the chain waits for a memory round trip it could have started earlier.
  auto load_l = [&](int J, int K, double (&a0)[8], double (&a1)[8]) {
    const double* lt = Sb + (size_t)(K * 32 + hi) * mld + J * 32 + lo;       // L[J][K], k-major: [contraction][row of J]
#pragma unroll
    for (int s8 = 0; s8 < 8; ++s8) { a0[s8] = lt[(size_t)(4 * s8) * mld]; a1[s8] = lt[(size_t)(4 * s8) * mld + 16]; }
  };
  auto load_linv = [&](int J, double (&l0)[4], double (&l1)[8]) {
    const double* li = Lb + (size_t)J * 1024 + hi * 32 + lo;                 // LinvT[p][k]: [contraction][row]
#pragma unroll
    for (int s8 = 0; s8 < 8; ++s8) { if (s8 < 4) l0[s8] = li[4 * s8 * 32]; l1[s8] = li[4 * s8 * 32 + 16]; }
  };
  v4d at[2];
  double li0[4], li1[8];
  double pa0[8], pa1[8];
  int pJ = wave + 1, pK = wave;                       // the wave's next (J, K)
  if (pJ < nblk) load_l(pJ, pK, pa0, pa1);
  if (wave == 0) {
#pragma unroll
    for (int jt = 0; jt < 2; ++jt)
#pragma unroll
      for (int r = 0; r < 4; ++r) at[jt][r] = Ab[(size_t)(16 * jt + hi + 4 * r) * ld + i0 + lo];
    load_linv(0, li0, li1);
  }
  for (int J = 0; J < nblk; ++J) {
    // ---- the products of this block row: K = wave, wave + 4, ...
    v4d acc[2];
    acc[0] = (v4d){0, 0, 0, 0};
    acc[1] = (v4d){0, 0, 0, 0};
    for (int K = wave; K < J; K += 4) {
      double a0[8], a1[8];
#pragma unroll
      for (int s8 = 0; s8 < 8; ++s8) { a0[s8] = pa0[s8]; a1[s8] = pa1[s8]; }
      // next pair: same block row while K + 4 < J, else the first product of the next block row that has one for this wave
      if (K + 4 < J) { pJ = J; pK = K + 4; } else { pJ = J + 1; pK = wave; }
      if (pJ < nblk) load_l(pJ, pK, pa0, pa1);
      const double* vk = &sV[K][hi * 16 + lo];
#pragma unroll
      for (int s8 = 0; s8 < 8; ++s8) {
        const double bv = vk[4 * s8 * 16];
        acc[0] = mfma_f64(a0[s8], bv, acc[0]);
        acc[1] = mfma_f64(a1[s8], bv, acc[1]);
      }
    }
#pragma unroll
    for (int jt = 0; jt < 2; ++jt)
#pragma unroll
      for (int r = 0; r < 4; ++r) sPart[wave][(16 * jt + hi + 4 * r) * 16 + lo] = acc[jt][r];
    __syncthreads();
    // ---- wave 0: rhs = At[J] - sum of the partial sums; V[J] = Linv_JJ rhs
    if (wave == 0) {
      v4d rhs[2];
#pragma unroll
      for (int jt = 0; jt < 2; ++jt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int e = (16 * jt + hi + 4 * r) * 16 + lo;
          rhs[jt][r] = at[jt][r] - (((sPart[0][e] + sPart[1][e]) + sPart[2][e]) + sPart[3][e]);
        }
      double l0[4], l1[8];
#pragma unroll
      for (int s8 = 0; s8 < 8; ++s8) { if (s8 < 4) l0[s8] = li0[s8]; l1[s8] = li1[s8]; }
      if (J + 1 < nblk) {          // the next block row of At and its inverted diagonal block travel under this product
#pragma unroll
        for (int jt = 0; jt < 2; ++jt)
#pragma unroll
          for (int r = 0; r < 4; ++r) at[jt][r] = Ab[(size_t)((J + 1) * 32 + 16 * jt + hi + 4 * r) * ld + i0 + lo];
        load_linv(J + 1, li0, li1);
      }
      v4d out[2];
      out[0] = (v4d){0, 0, 0, 0};
      out[1] = (v4d){0, 0, 0, 0};
#pragma unroll
      for (int s8 = 0; s8 < 8; ++s8) {
        const double bv = rhs[s8 >> 2][s8 & 3];
        if (s8 < 4) out[0] = mfma_f64(l0[s8], bv, out[0]);          // Linv lower triangular: rows 0..15 need p < 16
        out[1] = mfma_f64(l1[s8], bv, out[1]);
      }
#pragma unroll
      for (int jt = 0; jt < 2; ++jt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = 16 * jt + hi + 4 * r;
          sV[J][row * 16 + lo] = out[jt][r];
          Vb[(size_t)(J * 32 + row) * ld + i0 + lo] = out[jt][r];
        }
    }
    __syncthreads();
  }
}

// the one-launch substitution: k_fwdsub_lds<nb>, nb = the system's blocks (UpdatePlan::fwd_nb)
static int launch_fwdsub_lds(sl2_engine* e, int nb) {
  const int B = e->B;
  const dim3 grid(xcd_grid(e->ld / 64, B)), block(256);
  LaunchScope ls(e, "k_fwdsub_lds", true);
#define SL2_FWD_CASE(NBV)                                                                                           \
  case NBV:                                                                                                         \
    hipLaunchKernelGGL((k_fwdsub_lds<NBV>), grid, block, 0, e->stream, e->At, e->Vt, e->St, e->LinvT, e->m_gate, \
                       e->ld, e->mld, e->nblk_max, B, 0, 0, e->ld / 64, NBV);                                       \
    break;
  static_assert(kFwdLdsMaxBlocks == 13, "one case per instantiation the plan may name");
  switch (nb) {
    SL2_FWD_CASE(1) SL2_FWD_CASE(2) SL2_FWD_CASE(3) SL2_FWD_CASE(4) SL2_FWD_CASE(5) SL2_FWD_CASE(6) SL2_FWD_CASE(7)
    SL2_FWD_CASE(8) SL2_FWD_CASE(9) SL2_FWD_CASE(10) SL2_FWD_CASE(11) SL2_FWD_CASE(12) SL2_FWD_CASE(13)
    default: set_error("launch_fwdsub_lds: no k_fwdsub_lds of this many blocks"); return SL2_ERR_INVALID;
  }
#undef SL2_FWD_CASE
  SL2_HIP(hipGetLastError());
  return SL2_OK;
}

// ---------------------------------------------------------------------------
// k_fwd_gemm: At[R0 .. R0+256) -= L[R0 .. R0+256)[0 .. R0) * Vt[0 .. R0), the contribution of the already
// solved block rows to one group of eight block rows (R0 = 32 J0).  64x64 output tiles, four waves of 32x32,
// both operands streamed through double-buffered LDS in chunks of 16 k-rows like k_syrk (L is stored
// k-major in St, so both staging reads are row segments).
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256, 4) k_fwd_gemm(double* __restrict__ At, const double* __restrict__ Vt,
                                                  const double* __restrict__ St, const int* __restrict__ m_count, int ld, int mld,
                                                  int B, int J0, int nrt) {
  // nrt: 64-row tiles of the group (4 = eight block rows, 2 = four)
  int b, t;
  const int ntc = ld / 64;
  if (!xcd_map(nrt * ntc, B, &b, &t)) return;
  const int cnt = m_count[b];
  if (cnt == 0) return;
  const int mp = (2 * cnt + 31) / 32 * 32;
  const int R0 = J0 * 32;
  const int r0 = R0 + (t / ntc) * 64, c0 = (t % ntc) * 64;
  if (r0 >= mp) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lo = lane & 15, hi = lane >> 4;
  const int wi = (wave >> 1) * 32, wj = (wave & 1) * 32;
  double* Ab = At + (size_t)b * mld * ld;
  const double* Vb = Vt + (size_t)b * mld * ld;
  const double* Sb = St + (size_t)b * mld * mld;
  __shared__ double sAB[2][2][kSyrkKC * 64];
  v4d acc[2][2];
  for (int it = 0; it < 2; ++it) for (int jt = 0; jt < 2; ++jt) acc[it][jt] = (v4d){0, 0, 0, 0};
  // L[r0 + c][k] = St[k][r0 + c]: both operands are row segments
  kpanel_product(Sb + r0, (size_t)mld, Vb + c0, (size_t)ld, R0 / kSyrkKC, false, wi, wj, sAB, acc);
#pragma unroll
  for (int it = 0; it < 2; ++it)
#pragma unroll
    for (int jt = 0; jt < 2; ++jt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        double* q = Ab + (size_t)(r0 + wi + 16 * it + hi + 4 * r) * ld + c0 + wj + 16 * jt + lo;
        *q -= acc[it][jt][r];
      }
}

// the panel solve of the panel-wise Cholesky (launch_chol_panels, sl2_update_chol.hip), in place on S: the ntile 64-column tiles
// from column c0 on, against the nb blocks of the panel that starts at block p0; pb = the panel width the plan chose
int launch_panel_solve(sl2_engine* e, int pb, int p0, int c0, int ntile, int nb) {
  const int B = e->B;
  LaunchScope ls(e, "k_fwdsub_lds@chol", true);
  if (pb == 8)
    hipLaunchKernelGGL((k_fwdsub_lds<8>), dim3(xcd_grid(ntile, B)), dim3(256), 0, e->stream, e->St, e->St, e->St,
                       e->LinvT, e->m_gate, e->mld, e->mld, e->nblk_max, B, p0, c0, ntile, nb);
  else
    hipLaunchKernelGGL((k_fwdsub_lds<kCholPanelBlocks>), dim3(xcd_grid(ntile, B)), dim3(256), 0, e->stream, e->St, e->St, e->St,
                       e->LinvT, e->m_gate, e->mld, e->mld, e->nblk_max, B, p0, c0, ntile, nb);
  SL2_HIP(hipGetLastError());
  return SL2_OK;
}

// substitution in groups of g = eight or four block rows (UpdatePlan::fwd_group_rows), for systems of more than 13 blocks
static int launch_fwdsub_grouped(sl2_engine* e, int g) {
  const int B = e->B;
  for (int J0 = 0; J0 < e->nblk_max; J0 += g) {
    if (J0 > 0) {
      LaunchScope ls(e, "k_fwd_gemm", true);
      hipLaunchKernelGGL(k_fwd_gemm, dim3(xcd_grid((g / 2) * (e->ld / 64), B)), dim3(256), 0, e->stream, e->At, e->Vt, e->St,
                         e->m_gate, e->ld, e->mld, B, J0, g / 2);
      SL2_HIP(hipGetLastError());
    }
    LaunchScope ls(e, "k_fwdsub_lds", true);
    if (g == 4)
      hipLaunchKernelGGL((k_fwdsub_lds<4>), dim3(xcd_grid(e->ld / 64, B)), dim3(256), 0, e->stream, e->At, e->Vt, e->St, e->LinvT,
                         e->m_gate, e->ld, e->mld, e->nblk_max, B, J0, 0, e->ld / 64, 4);
    else
      hipLaunchKernelGGL((k_fwdsub_lds<8>), dim3(xcd_grid(e->ld / 64, B)), dim3(256), 0, e->stream, e->At, e->Vt, e->St, e->LinvT,
                         e->m_gate, e->ld, e->mld, e->nblk_max, B, J0, 0, e->ld / 64, 8);
    SL2_HIP(hipGetLastError());
  }
  return SL2_OK;
}

// V = A L^-T in the plan's form
int launch_substitute(sl2_engine* e, const UpdatePlan& p) {
  switch (p.fwd) {
    case FwdForm::kKsplit: {
      const int B = e->B;
      LaunchScope ls(e, "k_fwdsub_ksplit", true);
      hipLaunchKernelGGL(k_fwdsub_ksplit, dim3(xcd_grid(e->ld / 16, B)), dim3(256), 0, e->stream, e->At, e->Vt, e->St, e->LinvT,
                         e->m_gate, e->ld, e->mld, e->nblk_max, B);
      SL2_HIP(hipGetLastError());
    } return SL2_OK;
    case FwdForm::kLds: return launch_fwdsub_lds(e, p.fwd_nb);
    case FwdForm::kGrouped: return launch_fwdsub_grouped(e, p.fwd_group_rows);
    default: return kNoProductForm;
  }
}

}  // namespace sl2
