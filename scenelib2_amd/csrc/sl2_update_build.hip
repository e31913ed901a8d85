// EKF update, first phase: A = P H^T and S = H A + R in one pass (the algebra and the k-major storage: sl2_ekf_update.hip).
#include "sl2_update_dev.hpp"

namespace sl2 {

// ---------------------------------------------------------------------------
// k_build_AS: k_build_A and k_build_S (sl2_update_testing.hip) in one pass (state sizes up to 1024 columns): the rows of
// At are produced four features (eight rows) at a time, parked in LDS, and S = H A + R for those
// eight columns of S is formed from LDS before they are overwritten -- At is not read back from
// memory at all (k_build_S re-reads all of it: 0.8 GB per launch at batch 1024, 100 features).
// Thread i plays two roles: column i of At, and row a = i of H (its 10 non-zeros in registers).
// The summation order of every entry is that of the two separate kernels.
// (Measured slower: requesting the next batch's rows of P before the S phase of the current one with a second set of registers
// - 118 registers instead of 78, four waves per SIMD instead of six: 0.54 vs 0.33 ms.  The plain loop at full occupancy streams
// at 5.0-5.4 TB/s: what bounds it is the 1.5 KB a wavefront keeps in flight, not HBM - k_build_AS_ahead below is the form for
// launches of one workgroup per sequence; this one serves split launches, smaller batches' ranges and ld > 1024.)
// ---------------------------------------------------------------------------
// NQ: columns per thread (thread t owns columns t, t + 1024, ...: NQ = 1 for ld <= 1024, 2 up to 2048 - the 1280x720 /
// 500-feature configuration, ld = 1536); BATCH: features per LDS batch (2 * BATCH * ld doubles of LDS).
template <int NQ, int BATCH>
__global__ void __launch_bounds__(1024) k_build_AS(const double* __restrict__ P, const double* __restrict__ f_Hx,
                                                  const double* __restrict__ f_Hy, const double* __restrict__ f_nu,
                                                  const double* __restrict__ f_R, const int* __restrict__ succ_idx,
                                                  const int* __restrict__ m_count, double* __restrict__ At,
                                                  double* __restrict__ St, const int* __restrict__ f_hcol,
                                                  const int* __restrict__ pos_err_any, int N, int ld, int mld) {
  extern __shared__ double sAt[];   // [2 * BATCH][ld]
  const int b = blockIdx.x;
  const int cnt = m_count[b];
  if (cnt == 0) return;
  const int m = 2 * cnt, mp = (m + 31) / 32 * 32;
  const int t = threadIdx.x;        // blockDim.x * NQ >= ld; the S role below needs blockDim.x >= mp
  double* Ab = At + (size_t)b * mld * ld;
  double* Sb = St + (size_t)b * mld * mld;
  const double* Pb = P + (size_t)b * ld * ld;
  const int* sidx = succ_idx + (size_t)b * N;
  // the state columns feature f's dh_by_dy multiplies: its own, 13 + 3 f - unless the sequence carries the reference's
  // misplaced position_in_total_state_vector_ (Q28, feature.cpp:254 / monoslam.cpp:564): then what k_search_score looked up
  const int* hcol = (pos_err_any[b] != 0) ? f_hcol + (size_t)b * N : nullptr;
  // role "columns i of At"
  double pc[NQ][7];
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const int i = t + q * (int)blockDim.x;
#pragma unroll
    for (int c = 0; c < 7; ++c) pc[q][c] = (i >= ld) ? 0.0 : ((i < 13) ? Pb[(size_t)i * ld + c] : Pb[(size_t)c * ld + i]);
  }
  // role "row a = t of H"
  double hx[7], hy[3], Rn = 0.0;
  int posa = 0;
  if (t < m) {
    const int fa = sidx[t >> 1];
    const size_t fia = (size_t)b * N + fa;
    posa = hcol ? hcol[fa] : 13 + 3 * fa;
    // (Q28 with the block landing INSIDE the vehicle state, posa < 7: the reference's dh_by_dx_tot.block(...) = dh_by_dy
    // OVERWRITES those entries of dh_by_dxv, monoslam.cpp:562-565 - the overlapped pose coefficients do not count)
#pragma unroll
    for (int c = 0; c < 7; ++c) hx[c] = (hcol && (unsigned)(c - posa) < 3u) ? 0.0 : f_Hx[fia * 14 + (t & 1) * 7 + c];
#pragma unroll
    for (int c = 0; c < 3; ++c) hy[c] = f_Hy[fia * 6 + (t & 1) * 3 + c];
    Rn = f_R[fia];
  }
  // gridDim.y workgroups share a sequence (small batches: one workgroup walking all the features is a chain of ~25 HBM
  // round trips, 86 us at batch 1): each takes a contiguous range of feature batches = rows of At and columns of S
  const int nbatch = (cnt + BATCH - 1) / BATCH, per = (nbatch + (int)gridDim.y - 1) / (int)gridDim.y;
  const int jbeg = (int)blockIdx.y * per * BATCH;
  const int jend = (jbeg + per * BATCH < cnt) ? jbeg + per * BATCH : cnt;
  for (int j0 = jbeg; j0 < jend; j0 += BATCH) {
    const int nb = (jend - j0 < BATCH) ? jend - j0 : BATCH;
#pragma unroll
    for (int jj = 0; jj < BATCH; ++jj) {
      if (jj < nb) {
        const int f = sidx[j0 + jj];
        const size_t fi = (size_t)b * N + f;
        const int pos = hcol ? hcol[f] : 13 + 3 * f;
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
          const int i = t + q * (int)blockDim.x;
          if (i < ld) {
            double py[3];
#pragma unroll
            for (int c = 0; c < 3; ++c)
              py[c] = Pb[(size_t)(pos + c) * ld + i];
#pragma unroll
            for (int r = 0; r < 2; ++r) {
              double acc = 0.0;
#pragma unroll
              for (int c = 0; c < 7; ++c) acc += pc[q][c] * ((hcol && (unsigned)(c - pos) < 3u) ? 0.0 : f_Hx[fi * 14 + r * 7 + c]);
#pragma unroll
              for (int c = 0; c < 3; ++c) acc += py[c] * f_Hy[fi * 6 + r * 3 + c];
              if (i == ld - 1) acc = f_nu[fi * 2 + r];
              Ab[(size_t)(2 * (j0 + jj) + r) * ld + i] = acc;
              sAt[(2 * jj + r) * ld + i] = acc;
            }
          }
        }
      }
    }
    __syncthreads();
    if (t < mp) {
#pragma unroll
      for (int kk = 0; kk < 2 * BATCH; ++kk) {
        const int k = 2 * j0 + kk;
        if (kk < 2 * nb && (t | 31) >= k) {     // blocks on and below the block diagonal
          double v = 0.0;
          if (t < m) {
            const double* arow = sAt + kk * ld;
            double acc = 0.0;
#pragma unroll
            for (int c = 0; c < 7; ++c) acc += hx[c] * arow[c];
#pragma unroll
            for (int c = 0; c < 3; ++c) acc += hy[c] * arow[posa + c];
            if (t == k) acc += Rn;
            v = acc;
          }
          Sb[(size_t)k * mld + t] = v;
        }
      }
    }
    __syncthreads();
  }
  // padding: rows of At up to the 32-multiple are zero, S is the identity there
  if (blockIdx.y != 0) return;
  for (int k = m; k < mp; ++k) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int i = t + q * (int)blockDim.x;
      if (i < ld) Ab[(size_t)k * ld + i] = 0.0;
    }
    if (t < mp && (t | 31) >= k) Sb[(size_t)k * mld + t] = (t == k) ? 1.0 : 0.0;
  }
}

// ---------------------------------------------------------------------------
// k_build_AS_ahead: k_build_AS for launches of one workgroup per sequence (no split along the features), ld <= 1024, with a
// batch of rows of P in flight per thread.  What bounds k_build_AS there is not HBM but the bytes it keeps in flight: per feature
// it issues three row loads, then walks a chain of scalar loads (succ_idx, the feature's H coefficients behind the hcol test),
// waits for the rows and stores - four serial round trips per batch, 1.5 KB outstanding per wavefront.  Here
//   * the sequence's measurement table is staged in LDS once (per successful feature kAheadEntry doubles: Hx[2][7] with the Q28
//     overwrite already applied, Hy[2][3], nu[2], R, and the column pos its dh_by_dy multiplies), so neither role loads a
//     coefficient from memory inside the loop.  The column role reads a feature's entry with ONE LDS read per wavefront (lane l
//     holds double l) and takes each coefficient from its lane as a scalar; the S role reads its row of H from the table at the
//     top of each S phase, into registers the consumed rows of P have left, instead of holding it across the loop;
//   * the 3 * BATCH rows of a batch are one register window: as soon as a feature's three rows are consumed the same registers
//     are requested for the feature BATCH places on (the last feature's after the S phase, which needs its six registers), so
//     nine to twelve rows per thread are in flight all the time, the waits are counted (vmcnt(N), never 0 in the loop) and the
//     S phase runs under the next batch's loads.  The body of a full batch with a full batch behind it has no branch; the last
//     full batch, the partial batch and the padding rows are tails of their own.
// The rows of P are read once and At is next read by another launch: both are streaming accesses (load_stream / store_stream);
// the stores of S stay plain, the Cholesky reads them next (profiles/update_streams_ab.json).
// Same grid, same roles, and every entry of At and St is the expression of k_build_AS term by term (bit-identical:
// tests/test_gpu_build_as_ahead.py).
// Registers: 80, no spills - six wavefronts per SIMD, as k_build_AS.  Measured (HISTORY section 8, profiles/build_as_ahead_ab.json):
// a second window (the whole next batch requested before the current one is consumed) needs 93 registers, five wavefronts per
// SIMD, and is no faster than k_build_AS; coefficients read by all 64 lanes from one LDS address, or the S role's row of H
// re-read from LDS for each of its eight columns, cost more LDS cycles than the loads they replace.
// LDS: [2 * BATCH][ld] rows of At, then the table ([tab_cap][kAheadEntry]); one array (make_update_plan keeps the sum inside
// kAheadLdsMax so that four workgroups of the headline shape share a CU).
// ---------------------------------------------------------------------------
template <int BATCH>
struct AheadRows { double v[BATCH][3]; };

// the column in entry en of the measurement table (kept as an integer in the low word of double 23)
__device__ __forceinline__ int ahead_pos(const double* en) { return *(const int*)(en + 23); }

// the double held by lane l (a constant) of a wavefront, as a scalar
__device__ __forceinline__ double ahead_lane(double v, int l) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}

// element t of a row whose base is the same for the whole wavefront: a scalar base and a 32-bit lane offset, no address pair
// per access in vector registers (the empty asm pins the base to scalar registers: left alone, the compiler folds the lane
// offset into a vector copy of the sequence's base and adds the row to that, 64 bits per access)
typedef __attribute__((address_space(1))) double ahead_gdouble;
__device__ __forceinline__ ahead_gdouble* ahead_at(const double* row, int t) {
  unsigned long long a = (unsigned long long)row;
  asm("" : "+s"(a));
  return (ahead_gdouble*)(a + (unsigned)t * (unsigned)sizeof(double));
}

// rows pos .. pos + 2 of P, column t, for features j0 .. j0 + nb - 1 of the table (FULL: nb == BATCH, no test)
template <int BATCH, bool FULL>
__device__ __forceinline__ void ahead_load(AheadRows<BATCH>& w, const double* __restrict__ Pb, const double* tab, int j0, int nb,
                                           int ld, int t) {
#pragma unroll
  for (int jj = 0; jj < BATCH; ++jj) {
    if (FULL || jj < nb) {
      const int pos = __builtin_amdgcn_readfirstlane(ahead_pos(tab + (j0 + jj) * kAheadEntry));   // (uniform: a scalar row base)
#pragma unroll
      for (int c = 0; c < 3; ++c) w.v[jj][c] = load_stream(ahead_at(Pb + (size_t)(pos + c) * ld, t));
    }
  }
}

// rows 2 j0 .. 2 (j0 + nb) - 1 of At: to memory and to the LDS batch.  REFILL (a full batch with a full batch behind it): as
// soon as a feature's three rows of P are consumed, the same registers are requested for the feature BATCH places on
template <int BATCH, bool FULL, bool REFILL>
__device__ __forceinline__ void ahead_rows(AheadRows<BATCH>& w, const double (&pc)[7], const double* tab, const double* __restrict__ Pb,
                                           double* __restrict__ Ab, double* sAt, int j0, int nb, int ld, int t) {
#pragma unroll
  for (int jj = 0; jj < BATCH; ++jj) {
    if (FULL || jj < nb) {
      // the feature's entry of the table: one LDS read per wavefront (lane l holds double l), each coefficient then a scalar
      // taken from its lane - 64 lanes reading every coefficient from one address cost ten times the LDS cycles
      double en = 0.0;
      if ((t & 63) < kAheadEntry) en = tab[(j0 + jj) * kAheadEntry + (t & 63)];
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        double acc = 0.0;
#pragma unroll
        for (int c = 0; c < 7; ++c) acc += pc[c] * ahead_lane(en, r * 7 + c);
#pragma unroll
        for (int c = 0; c < 3; ++c) acc += w.v[jj][c] * ahead_lane(en, 14 + r * 3 + c);
        if (t == ld - 1) acc = ahead_lane(en, 20 + r);
        store_stream(ahead_at(Ab + (size_t)(2 * (j0 + jj) + r) * ld, t), acc);
        sAt[(2 * jj + r) * ld + t] = acc;
      }
      if (REFILL && jj < BATCH - 1) {      // (the last feature's registers are refilled behind the S phase: ahead_refill_last)
        const int pos = __builtin_amdgcn_readfirstlane(ahead_pos(tab + (j0 + BATCH + jj) * kAheadEntry));
#pragma unroll
        for (int c = 0; c < 3; ++c) w.v[jj][c] = load_stream(ahead_at(Pb + (size_t)(pos + c) * ld, t));
      }
    }
  }
}

// the rows of the last feature of the batch behind batch j0: requested after the S phase of batch j0, which has these six
// registers for its row of H (nine rows per thread are in flight through the S phase, twelve once it is over)
template <int BATCH>
__device__ __forceinline__ void ahead_refill_last(AheadRows<BATCH>& w, const double* tab, const double* __restrict__ Pb, int j0, int ld, int t) {
  const int pos = __builtin_amdgcn_readfirstlane(ahead_pos(tab + (j0 + 2 * BATCH - 1) * kAheadEntry));
#pragma unroll
  for (int c = 0; c < 3; ++c) w.v[BATCH - 1][c] = load_stream(ahead_at(Pb + (size_t)(pos + c) * ld, t));
}

// columns 2 j0 .. 2 (j0 + nb) - 1 of S from the LDS batch (between the two barriers of a batch)
template <int BATCH>
__device__ __forceinline__ void ahead_S(const double* sAt, const double* tab, double* __restrict__ Sb, int j0, int nb, int m, int mp,
                                        int ld, int mld, int t) {
  __syncthreads();
  // row a = t of H: read from the table once per batch, into registers the batch's rows of P have just left
  double hx[7], hy[3], Rn = 0.0;
  int posa = 0;
  if (t < m) {
    const double* en = tab + (t >> 1) * kAheadEntry;
#pragma unroll
    for (int c = 0; c < 7; ++c) hx[c] = en[(t & 1) * 7 + c];
#pragma unroll
    for (int c = 0; c < 3; ++c) hy[c] = en[14 + (t & 1) * 3 + c];
    Rn = en[22];
    posa = ahead_pos(en);
  }
#pragma unroll
  for (int kk = 0; kk < 2 * BATCH; ++kk) {
    const int k = 2 * j0 + kk;
    if (kk < 2 * nb) {
      const double* arow = sAt + kk * ld;
      if (t < mp && (t | 31) >= k) {     // blocks on and below the block diagonal
        double v = 0.0;
        if (t < m) {
          double acc = 0.0;
#pragma unroll
          for (int c = 0; c < 7; ++c) acc += hx[c] * arow[c];
#pragma unroll
          for (int c = 0; c < 3; ++c) acc += hy[c] * arow[posa + c];
          if (t == k) acc += Rn;
          v = acc;
        }
        Sb[(size_t)k * mld + t] = v;
      }
    }
  }
  __syncthreads();
}

template <int BATCH>
__global__ void __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(6, 8))) k_build_AS_ahead(const double* __restrict__ P, const double* __restrict__ f_Hx,
                                                        const double* __restrict__ f_Hy, const double* __restrict__ f_nu,
                                                        const double* __restrict__ f_R, const int* __restrict__ succ_idx,
                                                        const int* __restrict__ m_count, double* __restrict__ At,
                                                        double* __restrict__ St, const int* __restrict__ f_hcol,
                                                        const int* __restrict__ pos_err_any, int N, int ld, int mld, int tab_cap) {
  extern __shared__ double sAt[];   // [2 * BATCH][ld], then the table [tab_cap][kAheadEntry]
  const int b = blockIdx.x;
  int cnt = m_count[b];
  if (cnt == 0) return;
  cnt = cnt > tab_cap ? tab_cap : cnt;     // (cannot happen: m_gate <= nsel_max; nothing is written outside the table)
  const int m = 2 * cnt, mp = (m + 31) / 32 * 32;
  const int t = threadIdx.x;        // blockDim.x == ld; the S role needs blockDim.x >= mp
  double* Ab = At + (size_t)b * mld * ld;
  double* Sb = St + (size_t)b * mld * mld;
  const double* Pb = P + (size_t)b * ld * ld;
  double* tab = sAt + 2 * BATCH * ld;
  {   // the measurement table (see k_build_AS for pos and the Q28 overwrite of the pose coefficients)
    const int* sidx = succ_idx + (size_t)b * N;
    const int* hcol = (pos_err_any[b] != 0) ? f_hcol + (size_t)b * N : nullptr;
    for (int idx = t; idx < cnt * kAheadEntry; idx += (int)blockDim.x) {
      const int j = idx / kAheadEntry, el = idx - j * kAheadEntry;
      const int f = sidx[j];
      const size_t fi = (size_t)b * N + f;
      const int pos = hcol ? hcol[f] : 13 + 3 * f;
      double v;
      if (el < 14) v = (hcol && (unsigned)(el % 7 - pos) < 3u) ? 0.0 : f_Hx[fi * 14 + el];
      else if (el < 20) v = f_Hy[fi * 6 + (el - 14)];
      else if (el < 22) v = f_nu[fi * 2 + (el - 20)];
      else if (el == 22) v = f_R[fi];
      else v = __longlong_as_double((long long)pos);
      tab[idx] = v;
    }
  }
  // role "column t of At"
  double pc[7];
#pragma unroll
  for (int c = 0; c < 7; ++c) pc[c] = load_stream((t < 13) ? &Pb[(size_t)t * ld + c] : &Pb[(size_t)c * ld + t]);
  __syncthreads();
  const int nfull = cnt / BATCH, rem = cnt - nfull * BATCH;
  AheadRows<BATCH> w;
  if (nfull > 0) {
    ahead_load<BATCH, true>(w, Pb, tab, 0, BATCH, ld, t);
    int k = 0;
    for (; k + 1 < nfull; ++k) {      // a full batch with a full batch behind it: no branch
      ahead_rows<BATCH, true, true>(w, pc, tab, Pb, Ab, sAt, k * BATCH, BATCH, ld, t);
      ahead_S<BATCH>(sAt, tab, Sb, k * BATCH, BATCH, m, mp, ld, mld, t);
      ahead_refill_last<BATCH>(w, tab, Pb, k * BATCH, ld, t);
    }
    ahead_rows<BATCH, true, false>(w, pc, tab, Pb, Ab, sAt, k * BATCH, BATCH, ld, t);
    ahead_S<BATCH>(sAt, tab, Sb, k * BATCH, BATCH, m, mp, ld, mld, t);
  }
  if (rem > 0) {   // the partial batch
    ahead_load<BATCH, false>(w, Pb, tab, nfull * BATCH, rem, ld, t);
    ahead_rows<BATCH, false, false>(w, pc, tab, Pb, Ab, sAt, nfull * BATCH, rem, ld, t);
    ahead_S<BATCH>(sAt, tab, Sb, nfull * BATCH, rem, m, mp, ld, mld, t);
  }
  // padding: rows of At up to the 32-multiple are zero, S is the identity there
  for (int k = m; k < mp; ++k) {
    store_stream(&Ab[(size_t)k * ld + t], 0.0);
    if (t < mp && (t | 31) >= k) Sb[(size_t)k * mld + t] = (t == k) ? 1.0 : 0.0;
  }
}

// A = P H^T, S = H A + R in the plan's one-pass form (sl2_create admits maps of up to 2048 state columns / 512 measured features)
int launch_build(sl2_engine* e, const UpdatePlan& p) {
  const dim3 build_grid(e->B, p.build_nsplit), build_block(p.build_threads);
#define SL2_BUILD_CASE(FORM, KERNEL, ...)                                                                                     \
  case BuildForm::FORM: {                                                                                                     \
    LaunchScope ls(e, "k_build_AS", true);                                                                                    \
    hipLaunchKernelGGL(KERNEL, build_grid, build_block, (size_t)p.build_lds_bytes, e->stream, e->P, e->f_Hx, e->f_Hy,         \
                       e->f_nu, e->f_R, e->succ_idx, e->m_gate, e->At, e->St, e->f_hcol, e->pos_err_any, e->N, e->ld, e->mld, \
                       ##__VA_ARGS__);                                                                                        \
    SL2_HIP(hipGetLastError());                                                                                               \
  } break;
  switch (p.build) {
    SL2_BUILD_CASE(kAhead4, (k_build_AS_ahead<4>), e->nsel_max)
    SL2_BUILD_CASE(kAhead2, (k_build_AS_ahead<2>), e->nsel_max)
    SL2_BUILD_CASE(kAS14, (k_build_AS<1, kASBatch>))
    SL2_BUILD_CASE(kAS22, (k_build_AS<2, 2>))
    default: return kNoProductForm;
  }
#undef SL2_BUILD_CASE
  return SL2_OK;
}

}  // namespace sl2
