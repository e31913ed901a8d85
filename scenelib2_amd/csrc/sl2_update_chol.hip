// EKF update, second phase: S = L L^T, blocked Cholesky over 32x32 blocks (the algebra and the k-major storage:
// sl2_ekf_update.hip).
#include "sl2_update_dev.hpp"
#include "sl2_chol_diag.hpp"

namespace sl2 {

// ---------------------------------------------------------------------------
// 32 x 32 tile helpers of the one-launch Cholesky (k_chol_left below) and its panel kernels.  (The RIGHT-looking one-launch
// kernel of rounds 1-2, k_chol_fused4, is profiles/r06_retired_variants.patch.)
// ---------------------------------------------------------------------------
struct Tile32 {
  v4d f[2][2];   // f[kt][it][r] = element (k = 16 kt + 4 r + hi, i = 16 it + lo) of a k-major 32x32 tile
};

__device__ __forceinline__ Tile32 tile_load(const double* __restrict__ Sb, int mld, int k0, int i0, int lo, int hi) {
  Tile32 t;
#pragma unroll
  for (int kt = 0; kt < 2; ++kt)
#pragma unroll
    for (int it = 0; it < 2; ++it)
#pragma unroll
      for (int r = 0; r < 4; ++r) t.f[kt][it][r] = Sb[(size_t)(k0 + 16 * kt + hi + 4 * r) * mld + i0 + 16 * it + lo];
  return t;
}
__device__ __forceinline__ void tile_store(double* __restrict__ Sb, int mld, int k0, int i0, int lo, int hi, const Tile32& t) {
#pragma unroll
  for (int kt = 0; kt < 2; ++kt)
#pragma unroll
    for (int it = 0; it < 2; ++it)
#pragma unroll
      for (int r = 0; r < 4; ++r) Sb[(size_t)(k0 + 16 * kt + hi + 4 * r) * mld + i0 + 16 * it + lo] = t.f[kt][it][r];
}
// panel tile: out[k][i] = sum_p Linv[k][p] S[o+p][i0+i]
// `need` (wave-uniform) says which 16 x 16 quarters f[kt][it] of a tile are wanted, bit 2 kt + it: the tiles of the LAST block row
// of a system whose last block holds at most 16 real rows (m mod 32 in 1 .. 16: m = 200 is one) have their rows 16 .. 31 = the
// identity padding, whose products are zeros (kTileRowsLo); of a DIAGONAL tile the D wave reads the lower triangle only, so the
// quarter above the diagonal (kt = 1, it = 0) is never looked at (kTileDiag), and with a padded last block only the first quarter
// is (kTileDiagLo).  A 7-block system of 200 rows runs 58 instead of 77 tile operations' worth of MFMAs.
constexpr int kTileAll = 15, kTileRowsLo = 5, kTileDiag = 11, kTileDiagLo = 1;
__device__ __forceinline__ Tile32 tile_panel(const double* sLinv, const double* __restrict__ Sb, int mld, int o, int i0, int lo,
                                             int hi, int need) {
  double b0[8], b1[8];
#pragma unroll
  for (int s8 = 0; s8 < 8; ++s8) {
    b0[s8] = Sb[(size_t)(o + 4 * s8 + hi) * mld + i0 + lo];
    b1[s8] = (need & 10) ? Sb[(size_t)(o + 4 * s8 + hi) * mld + i0 + 16 + lo] : 0.0;
  }
  Tile32 t;
#pragma unroll
  for (int kt = 0; kt < 2; ++kt)
#pragma unroll
    for (int it = 0; it < 2; ++it) t.f[kt][it] = (v4d){0, 0, 0, 0};
#pragma unroll
  for (int s8 = 0; s8 < 8; ++s8) {
    const int p = 4 * s8 + hi;
    const double a0 = sLinv[p * kLinvPitch + lo], a1 = sLinv[p * kLinvPitch + 16 + lo];
    t.f[0][0] = mfma_f64(a0, b0[s8], t.f[0][0]);
    if (need & 2) t.f[0][1] = mfma_f64(a0, b1[s8], t.f[0][1]);
    t.f[1][0] = mfma_f64(a1, b0[s8], t.f[1][0]);
    if (need & 8) t.f[1][1] = mfma_f64(a1, b1[s8], t.f[1][1]);
  }
  return t;
}
// the same with the tile in registers: the fragment (k = 4 s8 + hi, i = 16 it + lo) of an accumulator IS the B operand of k-step s8
__device__ __forceinline__ Tile32 tile_panel_regs(const double* sLinv, const Tile32& in, int lo, int hi, int need) {
  Tile32 t;
#pragma unroll
  for (int kt = 0; kt < 2; ++kt)
#pragma unroll
    for (int it = 0; it < 2; ++it) t.f[kt][it] = (v4d){0, 0, 0, 0};
#pragma unroll
  for (int s8 = 0; s8 < 8; ++s8) {
    const int p = 4 * s8 + hi;
    const double a0 = sLinv[p * kLinvPitch + lo], a1 = sLinv[p * kLinvPitch + 16 + lo];
    const double b0 = in.f[s8 >> 2][0][s8 & 3], b1 = in.f[s8 >> 2][1][s8 & 3];
    t.f[0][0] = mfma_f64(a0, b0, t.f[0][0]);
    if (need & 2) t.f[0][1] = mfma_f64(a0, b1, t.f[0][1]);
    t.f[1][0] = mfma_f64(a1, b0, t.f[1][0]);
    if (need & 8) t.f[1][1] = mfma_f64(a1, b1, t.f[1][1]);
  }
  return t;
}

// ---------------------------------------------------------------------------
// k_chol_left: the LEFT-looking form of the one-launch factorisation.  A right-looking
// kernel reads and re-writes every trailing tile once per block column (1.6 GB of traffic per
// launch at batch 1024, m = 200, against 0.23 GB of matrix): here tile (I, J) is read once, updated
// with all its J products L[I][K] L[J][K]^T from finished columns, solved and written once.
// Per block column J (waves: D = 0, M0..M2 = 1..3), two barriers:
//   P2  D factors + inverts the diagonal block (from LDS) while the M waves update the tiles below it; M0 takes tile
//       (J+1, J) and also forms the next diagonal tile (J+1, J+1) up to its products K < J, parked in LDS             X2
//   P3  panel solves L[I][J] = T[I][J] L_JJ^-T; M0 solves (J+1, J) first, subtracts its square (still in registers)
//       from the next diagonal tile and leaves that in LDS in the layout D reads                                     X3
// (The first version updated the whole diagonal tile in a phase of its own at the top of the column, M0 alone with
// three waves waiting: 0.8 + 2.6 J kcycles of a 20-40 kcycle column, scripts/chol_trace.py.)
// ---------------------------------------------------------------------------
// (the D wave's routine - d_column: [A; I] -> [L; L^-T] by column Cholesky, a row per lane - lives in sl2_chol_diag.hpp, which the
// fused small-map kernel of sl2_small.hip shares)
// acc(I, J) -= sum_{K < kend} L[J][K-block] L[I][K-block]^T (kend = J: the complete left-looking update)
__device__ __forceinline__ Tile32 tile_left_update(double* __restrict__ Sb, int mld, int J, int I, int kend, int lo, int hi, int need) {
  Tile32 acc = tile_load(Sb, mld, J * 32, I * 32, lo, hi);
  // (measured slower: an explicit register prefetch of the next half-step's operands, 0.275 vs 0.243 ms; all 32 operand
  // loads of a product in one batch, 0.271 vs 0.266)
  for (int K = 0; K < kend; ++K) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      double a0[4], a1[4], b0[4], b1[4];
#pragma unroll
      for (int s4 = 0; s4 < 4; ++s4) {
        const size_t row = (size_t)(K * 32 + 16 * h + 4 * s4 + hi) * mld;
        a0[s4] = Sb[row + J * 32 + lo];
        a1[s4] = (need & 12) ? Sb[row + J * 32 + 16 + lo] : 0.0;
        b0[s4] = Sb[row + I * 32 + lo];
        b1[s4] = (need & 10) ? Sb[row + I * 32 + 16 + lo] : 0.0;
      }
#pragma unroll
      for (int s4 = 0; s4 < 4; ++s4) {
        acc.f[0][0] = mfma_f64(-a0[s4], b0[s4], acc.f[0][0]);
        if (need & 2) acc.f[0][1] = mfma_f64(-a0[s4], b1[s4], acc.f[0][1]);
        if (need & 4) acc.f[1][0] = mfma_f64(-a1[s4], b0[s4], acc.f[1][0]);
        if (need & 8) acc.f[1][1] = mfma_f64(-a1[s4], b1[s4], acc.f[1][1]);
      }
    }
  }
  return acc;
}
// diagonal tile: acc -= l^T l for the k-major panel tile l = L[I][J-block] held in registers (A and B fragments coincide)
__device__ __forceinline__ void tile_diag_sub_regs(Tile32& acc, const Tile32& l, int need) {
#pragma unroll
  for (int s8 = 0; s8 < 8; ++s8) {
    const double v0 = l.f[s8 >> 2][0][s8 & 3], v1 = l.f[s8 >> 2][1][s8 & 3];
    acc.f[0][0] = mfma_f64(-v0, v0, acc.f[0][0]);
    if (need & 2) acc.f[0][1] = mfma_f64(-v0, v1, acc.f[0][1]);
    if (need & 4) acc.f[1][0] = mfma_f64(-v1, v0, acc.f[1][0]);
    if (need & 8) acc.f[1][1] = mfma_f64(-v1, v1, acc.f[1][1]);
  }
}

__global__ void __launch_bounds__(256, 4) k_chol_left(double* __restrict__ St, double* __restrict__ LinvT,
                                                      const int* __restrict__ m_count, int mld, int nblk_max, int J0, int nb_cap,
                                                      long long* trace) {
  // J0 / nb_cap: factor the diagonal sub-matrix of blocks J0 .. J0 + nb_cap - 1 only (panel-wise factorisation of
  // large systems, launch_chol_panels); block indices below are relative to J0.  (0, any) = the whole matrix.
  const int b = blockIdx.x;
  const int cnt = m_count[b];
  if (cnt == 0) return;
  int nblk = (2 * cnt + 31) / 32 - J0;
  if (nblk <= 0) return;
  if (nblk > nb_cap) nblk = nb_cap;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool isD = wave == 0;
  const int mw = wave - 1;
  // the last block of THIS launch holds at most 16 real rows (its rows 16 .. 31 are the identity padding): see kTileRowsLo
  const bool half_last = 2 * cnt - 32 * (J0 + nblk - 1) <= 16;
  auto off_need = [&](int I) { return (half_last && I == nblk - 1) ? kTileRowsLo : kTileAll; };
  auto diag_need = [&](int I) { return (half_last && I == nblk - 1) ? kTileDiagLo : kTileDiag; };
  __shared__ double sTile[32][33];
  __shared__ double sLinv[32 * kLinvPitch];
  __shared__ double sNext[1024];      // the next diagonal tile (partial), MFMA fragment order
  __shared__ __attribute__((aligned(16))) double sCol[2][64];   // the D wave's last two columns of L (scalar operands of its products)
  __shared__ double sIdent[32][33];   // the identity the D wave starts its inverse from
  double* Sb = St + (size_t)b * mld * mld + (size_t)J0 * 32 * mld + J0 * 32;
  LinvT += (size_t)J0 * 1024;
#ifdef SL2_CHOL_TRACE
#define TRL(slot) do { if (trace && lane == 0 && J < 8) trace[(((size_t)b * 4 + wave) * 8 + J) * 4 + (slot)] = (long long)__builtin_readcyclecounter(); } while (0)
#else
#define TRL(slot) do { } while (0)
#endif
#ifdef SL2_CHOL_TRACE
  if (trace && lane == 0) trace[(size_t)gridDim.x * 4 * 8 * 4 + b * 4 + wave] = __builtin_amdgcn_s_getreg(63492);   // HW_ID
#endif
  // (Wave 0 = D of consecutive workgroups already lands on rotating SIMDs - 250 / 255 / 257 / 262 of 1024 per SIMD - ; an
  // explicit per-CU ticket that picks the D wave by SIMD id made the launch 6 % slower.)
  auto diag_to_lds = [&](const Tile32& t, int lo, int hi) {
#pragma unroll
    for (int jt = 0; jt < 2; ++jt)
#pragma unroll
      for (int it = 0; it < 2; ++it)
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) sTile[16 * it + lo][16 * jt + hi + 4 * r4] = t.f[jt][it][r4];
  };
  if (mw == 0) diag_to_lds(tile_load(Sb, mld, 0, 0, lane & 15, lane >> 4), lane & 15, lane >> 4);
  for (int i = threadIdx.x; i < 32 * 33; i += 256) (&sIdent[0][0])[i] = (i / 33 == i % 33) ? 1.0 : 0.0;
  __syncthreads();
  for (int J = 0; J < nblk; ++J) {
    const int o = J * 32;
    int lane_j = lane;
    asm volatile("" : "+v"(lane_j));      // (a copy the compiler cannot hoist: as a loop-carried value of the J loop it cost six spilled registers, round 2)
    const int lo = lane_j & 15, hi = lane_j >> 4;
    const bool more = J + 1 < nblk;
    TRL(0);
    TRL(1);
    // P3 for the tiles that went through memory (tasks 3, 5, 6, 7, ...): the D wave (idle in that phase), M1 and M2 in turn
    auto solve_stored = [&](int turn) {
      for (int sidx = turn; ; sidx += 3) {
        const int t = sidx == 0 ? 3 : sidx + 4;
        if (J + t >= nblk) break;
        const Tile32 u = tile_panel(sLinv, Sb, mld, o, (J + t) * 32, lo, hi, off_need(J + t));
        tile_store(Sb, mld, o, (J + t) * 32, lo, hi, u);
      }
    };
    // ---- P2 ----
    if (isD) {
      // the diagonal factorisation is the critical path of the whole kernel (its wave shares a SIMD with MFMA waves of
      // other sequences and was measured 2x slower under that contention): let the scheduler prefer it
      __builtin_amdgcn_s_setprio(3);
      const int r = lane_j & 31;
      const bool low = lane_j < 32;
      double a[32];
      const double* src = low ? &sTile[r][0] : &sIdent[r][0];
#pragma unroll
      for (int c = 0; c < 32; ++c) a[c] = src[c];
      // rows of L^-T (lanes 32..63) go to sLinv as their columns finish; the rows of L, which nobody reads, back into sTile
      double* rows = low ? &sTile[r][0] : &sLinv[r * kLinvPitch];
      DScal t;
      t.s = 0.0;
      d_column<0>(a, t, (unsigned)(size_t)(__attribute__((address_space(3))) double*)&sCol[0][0], &sCol[0][lane_j], rows);
      rows[31] = a[31];
      __builtin_amdgcn_s_setprio(0);
      TRL(2);
      __syncthreads();                     // X2: L_JJ^-1 is in LDS, every tile of column J is updated
      solve_stored(0);
    } else {
      // The column's update tasks - 0: tile (J+1, J); 1: the next diagonal tile (J+1, J+1) as far as finished columns go;
      // t >= 2: tile (J+t, J) - are dealt M0, M1, M2, M0, ...: every task costs J tile products, so this is what balances the
      // three waves.  (M0 used to take (J+1, J) AND the next diagonal tile on top of its share of the others: 3 / 1 / 1 tasks
      // at J = 2, 2 / 0 / 0 at J = 5, and its 40-60 k cycles were the column's critical path next to 20-30 k for M1 / M2.)
      // The next diagonal tile is parked in LDS in fragment order (held in registers across the barrier and the panel solve
      // it spilled); M0 picks it up in P3.
      // Round 3: a wave's FIRST tile (tasks 0 / 4 / 2 of M0 / M1 / M2) is updated last and stays in its registers across X2 -
      // the accumulator fragment of the update is the B fragment of the panel solve - instead of going out to memory and
      // coming back: 14 of a 7-block system's 21 tiles, 0.24 MB of a sequence's 1.1 MB of traffic in a bandwidth-bound
      // kernel, and one store -> barrier -> load round trip less on M0's chain.
      Tile32 kept;                         // the wave's first tile of the column, from its update to its solve
#pragma unroll
      for (int q = 0; q < 4; ++q) kept.f[q >> 1][q & 1] = (v4d){0, 0, 0, 0};   // (left undefined it becomes a value carried around the J loop: 86 spilled registers)
      int keptI = nblk;
      if (more) {                                   // (the last column has no tile below it)
        if (mw == 1) {                              // task 1
          const Tile32 dn = tile_left_update(Sb, mld, J + 1, J + 1, J, lo, hi, diag_need(J + 1));
#pragma unroll
          for (int k = 0; k < 16; ++k) sNext[k * 64 + lane_j] = dn.f[k >> 3][(k >> 2) & 1][k & 3];
        }
        const int t_keep = mw == 0 ? 0 : (mw == 1 ? 4 : 2);
        for (int t = t_keep + 3; J + t < nblk; t += 3) {          // the wave's later tiles: updated, stored
          const Tile32 u = tile_left_update(Sb, mld, J, J + t, J, lo, hi, off_need(J + t));
          tile_store(Sb, mld, o, (J + t) * 32, lo, hi, u);
        }
        keptI = mw == 0 ? J + 1 : J + t_keep;
        if (keptI < nblk) kept = tile_left_update(Sb, mld, J, keptI, J, lo, hi, off_need(keptI));
      }
      TRL(2);
      __syncthreads();                     // X2 (the D wave meets it in its own branch)
      // ---- P3 ----
      if (keptI < nblk) {
        const Tile32 l = tile_panel_regs(sLinv, kept, lo, hi, off_need(keptI));
        tile_store(Sb, mld, o, keptI * 32, lo, hi, l);
        if (mw == 0) {                     // the chain: the next diagonal tile minus the square of the tile just solved
          Tile32 dn;
#pragma unroll
          for (int q = 0; q < 16; ++q) dn.f[q >> 3][(q >> 2) & 1][q & 3] = sNext[q * 64 + lane_j];
          tile_diag_sub_regs(dn, l, diag_need(J + 1));
          diag_to_lds(dn, lo, hi);
        }
      }
      if (mw == 2) {   // LinvT block to memory for the forward substitution, coalesced
        double* Lb = LinvT + ((size_t)b * nblk_max + J) * 1024;
#pragma unroll
        for (int q = 0; q < 16; ++q) Lb[q * 64 + lane_j] = sLinv[(q * 2 + (lane_j >> 5)) * kLinvPitch + (lane_j & 31)];
      }
      if (mw >= 1) solve_stored(mw);       // M0 keeps to the chain above
    }
    TRL(3);
    if (more) __syncthreads();             // X3: column J of L is complete, the next diagonal tile is in LDS
  }
}
#undef TRL

// ---------------------------------------------------------------------------
// Cholesky of systems with more than 16 blocks (launch_chol_panels): right-looking over PANELS of eight block columns
// (256 columns; four in rounds 1-2), so that the trailing matrix is read and written once per panel instead of once per 32
// columns (the launch-per-block kernels are bound by exactly that traffic: 22 GB per factorisation at m = 1000, batch 256):
//   k_chol_left (J0, 8 blocks)      factor the 256x256 diagonal sub-matrix in one launch
//   k_fwdsub_lds<8> on S itself     panel solve X = S[below][panel] L_dd^-T  (S is k-major: the panel's columns are rows
//                                   of St, i.e. exactly the right-hand-side layout of the EKF substitution;
//                                   launch_panel_solve, sl2_update_fwdsub.hip)
//   k_chol_syrk                     S[below][below] -= X X^T, 64x64 tiles of the lower block triangle, K = 256
// (with K = 128 a tile of the trailing update had eight K-chunks to amortise its read-modify-write over: 38 TFLOP/s)
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_chol_syrk(double* __restrict__ St, const int* __restrict__ m_count, int mld, int B,
                                                   int k0, int kp, int c0) {
  int b, t;
  const int nt = (mld - c0) / 64;
  if (!xcd_map(nt * (nt + 1) / 2, B, &b, &t)) return;
  const int cnt = m_count[b];
  if (cnt == 0) return;
  const int mp = (2 * cnt + 31) / 32 * 32;
  int ti = 0;
  while (t > ti) { t -= ti + 1; ++ti; }
  const int tj = t;                       // tj <= ti : column block j <= row block i (lower triangle, stored St[j][i])
  const int j0 = c0 + tj * 64, i0 = c0 + ti * 64;
  if (j0 >= mp || i0 >= mp) return;       // (j0 <= i0; tiles of the padding are never read)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lo = lane & 15, hi = lane >> 4;
  const int wj = (wave >> 1) * 32, wi = (wave & 1) * 32;
  double* Sb = St + (size_t)b * mld * mld;
  __shared__ double sAB[2][2][kSyrkKC * 64];
  v4d acc[2][2];
  for (int a = 0; a < 2; ++a) for (int c = 0; c < 2; ++c) acc[a][c] = (v4d){0, 0, 0, 0};
  // rows of the panel beyond this sequence's own (padded) system are never initialised: stop at mp
  const int kvalid = (mp - k0 < kp) ? mp - k0 : kp;
  // in a diagonal tile the block (rows j0 + 32 .., columns i0 ..) lies above the diagonal: nobody reads it
  const bool idle = (ti == tj) && (wj > wi);
  // X[j0 + c][k] = St[k][j0 + c]
  kpanel_product(Sb + (size_t)k0 * mld + j0, (size_t)mld, Sb + (size_t)k0 * mld + i0, (size_t)mld, kvalid / kSyrkKC, idle, wj, wi, sAB,
                 acc);
  if (idle) return;
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        double* q = Sb + (size_t)(j0 + wj + 16 * a + hi + 4 * r) * mld + i0 + wi + 16 * c + lo;
        *q -= acc[a][c][r];
      }
}

// the large-map Cholesky in panels of pb 32-blocks (UpdatePlan::chol_panel_blocks: kCholPanelBlocks or 8)
static int launch_chol_panels(sl2_engine* e, int pb) {
  const int B = e->B;
  for (int p0 = 0; p0 < e->nblk_max; p0 += pb) {
    const int nb = e->nblk_max - p0 < pb ? e->nblk_max - p0 : pb;
    {
      LaunchScope ls(e, "k_chol_left", true);
      hipLaunchKernelGGL(k_chol_left, dim3(B), dim3(256), 0, e->stream, e->St, e->LinvT, e->m_gate, e->mld, e->nblk_max, p0, nb,
                         (long long*)nullptr);
      SL2_HIP(hipGetLastError());
    }
    const int c0 = (p0 + nb) * 32;
    if (c0 >= e->mld) break;
    const int ntile = (e->mld - c0) / 64;      // mld is a multiple of 64 for these sizes (sl2_create)
    const int rc = launch_panel_solve(e, pb, p0, c0, ntile, nb);
    if (rc != SL2_OK) return rc;
    {
      LaunchScope ls(e, "k_chol_syrk", true);
      hipLaunchKernelGGL(k_chol_syrk, dim3(xcd_grid(ntile * (ntile + 1) / 2, B)), dim3(256), 0, e->stream, e->St, e->m_gate, e->mld,
                         B, p0 * 32, nb * 32, c0);
      SL2_HIP(hipGetLastError());
    }
  }
  return SL2_OK;
}

// S = L L^T in the plan's form
int launch_factor(sl2_engine* e, const UpdatePlan& p) {
  switch (p.chol) {
    case CholForm::kPanels: return launch_chol_panels(e, p.chol_panel_blocks);
    case CholForm::kLeft: {
      LaunchScope ls(e, "k_chol_left", true);
      hipLaunchKernelGGL(k_chol_left, dim3(e->B), dim3(256), 0, e->stream, e->St, e->LinvT, e->m_gate, e->mld, e->nblk_max, 0,
                         e->nblk_max, (long long*)e->root->chol_trace);
      SL2_HIP(hipGetLastError());
    } return SL2_OK;
    default: return kNoProductForm;
  }
}

}  // namespace sl2
