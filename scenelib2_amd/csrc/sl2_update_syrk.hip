// EKF update, last phase: P -= V V^T, x += V (L^-1 nu) (the algebra and the k-major storage: sl2_ekf_update.hip).
#include "sl2_update_dev.hpp"

namespace sl2 {

// ---------------------------------------------------------------------------
// k_syrk: P -= V V^T on 64x64 tiles of the upper block triangle (ti <= tj),
// mirrored to the lower one; 4 waves per tile, 32x32 per wave.  The column
// ld-1 of Vt is w = L^-1 nu, so the same product yields x += V w there.
//
// The two 64-column panels of V^T are streamed through LDS in K-chunks of 16 rows,
// double-buffered: the global loads of chunk c+1 are in flight while the 16 MFMAs
// of chunk c run (the kernel was memory-latency-bound with direct fragment loads:
// SQ_WAIT_ANY 55 %, MFMA pipe 38 % busy).  LDS: 32 KB, rows of 64 doubles without padding; the odd k-rows swap their
// two 16-column halves within each 32-column group (column ^ 16), so that the two k-rows read by one 32-lane group of a
// ds_read_b64 land on disjoint banks (the first version padded the rows to 80 doubles: 40 KB, three workgroups per CU).
// ---------------------------------------------------------------------------

__global__ void __launch_bounds__(256, 4) k_syrk(const double* __restrict__ Vt, double* __restrict__ P, double* __restrict__ x,
                                              const int* __restrict__ m_count, int ld, int mld, int B,
                                              const int* __restrict__ n_slots, int ppos
#ifdef SL2_CHOL_TRACE
                                              , long long* trace
#endif
                                              ) {
#ifdef SL2_CHOL_TRACE   // development builds: entry / exit cycle stamps of wave 0 (scripts/syrk_clock.py)
  struct Stamp {
    long long* p;
    __device__ Stamp(long long* q) : p(q) { if (p && threadIdx.x == 0) p[2 * blockIdx.x] = (long long)__builtin_readcyclecounter(); }
    __device__ ~Stamp() { if (p && threadIdx.x == 0) p[2 * blockIdx.x + 1] = (long long)__builtin_readcyclecounter(); }
  } stamp(trace);
#endif
  int b, t;
  const int ntl = ld / 64;
  if (!xcd_map(ntl * (ntl + 1) / 2, B, &b, &t)) return;
  const int cnt = m_count[b];
  if (cnt == 0) return;
  const int mp = (2 * cnt + kSyrkKC - 1) / kSyrkKC * kSyrkKC;   // rows >= 2 cnt of Vt are zero up to the 16-multiple
  // k-steps (of 4 rows) of the LAST chunk that hold measurements: with m = 198 the 13th chunk has 6 live rows of 16,
  // and the two k-steps of zeros were 3 % of the launch's matrix instructions
  const int nks_last = (2 * cnt - (mp - kSyrkKC) + 3) >> 2;
  int tj = 0;
  while (t > tj) { t -= tj + 1; ++tj; }
  const int ti = t;  // ti <= tj
  // The engine's P has room for max_features slots; the columns of slots a sequence has never used - between its last slot
  // and the partially initialised features at ppos - are zero in P and in V^T, and a tile that lies in them has nothing to
  // subtract: with mapping on, a map that has grown to a third of its capacity pays for a ninth of the tiles (at 84-100
  // live features of 200: 21 tiles of 55, k_syrk 1.04 -> 0.43 ms, profiles/r04_live_tiles.txt).
  const int n_live = 13 + 3 * n_slots[b];
  {
    const int t_lo = (n_live + 63) >> 6, t_hi = ppos >> 6;
    if ((ti >= t_lo && ti < t_hi) || (tj >= t_lo && tj < t_hi)) return;
  }
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int lo = lane & 15, hi = lane >> 4;
  const int wi = (wave >> 1) * 32, wj = (wave & 1) * 32;
  const double* Vb = Vt + (size_t)b * mld * ld;
  double* Pb = P + (size_t)b * ld * ld;
  // LDS: [buffer][A | B][16 k-rows x 64 columns], 32 KB (the 80-double row pitch of the first version cost 40 KB = three
  // workgroups per CU: with m = 200 a tile has only 13 chunks, and a third of its life is prologue and epilogue, which
  // only other resident workgroups can cover).  Registers: 76 + 32 accumulator = 108 -> FOUR workgroups per CU; forcing
  // five (__launch_bounds__(256, 5): 94 registers, no spills) measured 0.507 against 0.498 ms, so four it stays.  Instead of padding, the odd k-rows swap their two
  // 16-column halves within each 32-column group (column ^ 16): the two k-rows read by one 32-lane group still land on
  // disjoint banks.
  __shared__ double sAB[2][2][kSyrkKC * 64];
  // staging role of this thread: row kr of the chunk, columns c2, c2+1 and 32+c2, 33+c2: sixteen lanes write 256
  // CONTIGUOUS bytes per ds_write_b128 (four consecutive doubles per lane put lanes 0 and 8 of a row on the same banks:
  // 2.6e7 conflict cycles per launch, three per LDS instruction)
  const int kr = tid >> 4, c2 = (tid & 15) * 2;
  const double* gA = Vb + (size_t)kr * ld + ti * 64 + c2;
  const double* gB = Vb + (size_t)kr * ld + tj * 64 + c2;
  struct Stage { double2 a0, a1, b0, b1; };
  auto stage_load = [&](int chunk) {
    Stage r;
    const size_t off = (size_t)chunk * kSyrkKC * ld;
    r.a0 = *(const double2*)(gA + off); r.a1 = *(const double2*)(gA + off + 32);
    r.b0 = *(const double2*)(gB + off); r.b1 = *(const double2*)(gB + off + 32);
    return r;
  };
  auto stage_store = [&](int buf, const Stage& r) {
    const int cs = c2 ^ ((kr & 1) << 4);
    *(double2*)&sAB[buf][0][kr * 64 + cs] = r.a0;
    *(double2*)&sAB[buf][0][kr * 64 + 32 + cs] = r.a1;
    *(double2*)&sAB[buf][1][kr * 64 + cs] = r.b0;
    *(double2*)&sAB[buf][1][kr * 64 + 32 + cs] = r.b1;
  };
  Stage r0 = stage_load(0);
  // In a diagonal tile the sub-block (wi = 32, wj = 0) is the mirror of (0, 32): that wave only stages.  So does a wave whose
  // 32 rows or 32 columns lie in never-used slots (the same rule as for whole tiles above, at the wavefront's granularity:
  // in the mapping workload - 128 columns of capacity, ~55 live, the partially initialised feature at 109 - nine of the
  // sixteen 32 x 32 blocks are live).
  const int i0 = ti * 64 + wi, j0 = tj * 64 + wj;
  const int b_lo = (n_live + 31) >> 5, b_hi = ppos >> 5;
  const bool idle = ((ti == tj) && (wi > wj)) || ((i0 >> 5) >= b_lo && (i0 >> 5) < b_hi) || ((j0 >> 5) >= b_lo && (j0 >> 5) < b_hi);
  v4d acc[2][2];
  for (int it = 0; it < 2; ++it) for (int jt = 0; jt < 2; ++jt) acc[it][jt] = (v4d){0, 0, 0, 0};
  const int nchunk = mp / kSyrkKC;
  // register prefetch runs TWO chunks ahead of the MFMAs (one chunk of work does not cover an
  // HBM round trip under load); chunks alternate between the register sets r0 / r1.
  Stage r1 = r0;
  if (nchunk > 1) r1 = stage_load(1);
  // The two diagonal 32x32 blocks of a diagonal tile are symmetric: their lower-left 16x16 quarter is not computed, the
  // epilogue writes it as the transpose of the upper-right one (interior blocks only: the innovation row / column of the
  // last block keeps the general path).
  const bool interior = (i0 + 32 < ld && j0 + 32 < ld);
  const bool diagw = (ti == tj) && (wi == wj) && interior;
  auto chunk_mfma = [&](int buf, int nks) {
    // k-row 4 ks + hi has the parity of hi: its first / second 16 columns sit at sw / sw ^ 16
    const int sw = (hi & 1) << 4;
    const double* pa = &sAB[buf][0][hi * 64 + wi + lo];
    const double* pb = &sAB[buf][1][hi * 64 + wj + lo];
#pragma unroll
    for (int ks = 0; ks < kSyrkKC / 4; ++ks) {
      if (ks < nks) {
        const double a0 = pa[ks * 256 + sw], a1 = pa[ks * 256 + (sw ^ 16)];
        const double b0 = pb[ks * 256 + sw], b1 = pb[ks * 256 + (sw ^ 16)];
        acc[0][0] = mfma_f64(a0, b0, acc[0][0]);
        acc[0][1] = mfma_f64(a0, b1, acc[0][1]);
        if (!diagw) acc[1][0] = mfma_f64(a1, b0, acc[1][0]);
        acc[1][1] = mfma_f64(a1, b1, acc[1][1]);
      }
    }
  };
  // The P tile of an interior block is fetched in one burst right after the K loop.  (Fetching it under the MFMAs of the
  // last chunk gained 2 % at three workgroups per CU, but holds 32 more registers through the loop: with the 32 KB LDS
  // layout the kernel is better off without the 32 extra registers, 0.535 vs 0.552 ms.  Peeling the last
  // chunk out of the loop made the compiler copy the prefetch registers and wait for every load on the spot: 1.40 ms.)
  double pold[2][2][4];
  auto fetch_tile = [&]() {
    const double* prow = Pb + (size_t)(i0 + hi) * ld + j0 + lo;
#pragma unroll
    for (int it = 0; it < 2; ++it)
#pragma unroll
      for (int jt = 0; jt < 2; ++jt)
#pragma unroll
        for (int r = 0; r < 4; ++r) pold[it][jt][r] = prow[(size_t)(16 * it + 4 * r) * ld + 16 * jt];
  };
  const bool want_tile = !idle;
  for (int ch = 0; ch < nchunk; ch += 2) {
    // even chunk: registers r0 -> buffer 0
    stage_store(0, r0);
    __syncthreads();
    if (ch + 2 < nchunk) r0 = stage_load(ch + 2);
    if (!idle) chunk_mfma(0, (ch + 1 >= nchunk) ? nks_last : kSyrkKC / 4);
    if (ch + 1 >= nchunk) break;
    // odd chunk: registers r1 -> buffer 1
    stage_store(1, r1);
    __syncthreads();
    if (ch + 3 < nchunk) r1 = stage_load(ch + 3);
    if (!idle) chunk_mfma(1, (ch + 2 >= nchunk) ? nks_last : kSyrkKC / 4);
    // a buffer is rewritten two chunks after it was read, with a barrier in between: one barrier per chunk suffices
  }
  const int lastbuf = (nchunk - 1) & 1;
  if (want_tile) fetch_tile();
  if (idle) return;
  const bool mirror = (ti != tj) || (wi != wj);
  // Row / column ld-1 (the innovation column riding along) only exists in the last tile row / column, and there only in the
  // last 16 x 16 quarter of a wave's block: every other quarter takes the branch-free path.  (Rounds 1-2 sent the whole
  // 32x32 block of such a wave - 40 of a sequence's 210 quarters, 20 of which hold the column - down the element-wise path
  // with its uncoalesced mirror stores.)
  auto plain = [&](int it, int jt) { return interior || ((i0 + 16 * it + 16 < ld) && (j0 + 16 * jt + 16 < ld)); };
  {
    double* prow = Pb + (size_t)(i0 + hi) * ld + j0 + lo;       // element (i0 + hi, j0 + lo)
#pragma unroll
    for (int it = 0; it < 2; ++it)
#pragma unroll
      for (int jt = 0; jt < 2; ++jt) {
        if (!plain(it, jt)) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          if (diagw && it == 1 && jt == 0) continue;            // written below as the transpose of quarter (0, 1)
          const double pn = pold[it][jt][r] - acc[it][jt][r];
          prow[(size_t)(16 * it + 4 * r) * ld + 16 * jt] = pn;
          acc[it][jt][r] = pn;
        }
      }
    if (mirror || diagw) {
      // The mirror block goes through LDS so that its stores are row segments of 128 bytes like the direct ones (written
      // straight from the accumulator layout every store instruction touched 16 rows with 32 bytes each: the mirror cost
      // 0.07 ms of the 0.58 ms launch).  The staging buffer that the LAST chunk did not use is free: every wave is past
      // the barrier that followed its last read.  Wave-private region, LDS operations of a wave execute in order.
      const int other = lastbuf ^ 1;
      double* sM = &sAB[other][0][0] + wave * (16 * 17);          // 16 x 16 block at pitch 17, one per wave
      double* pm = Pb + (size_t)(j0 + hi) * ld + i0 + lo;       // element (j0 + hi, i0 + lo)
#pragma unroll
      for (int it = 0; it < 2; ++it)
#pragma unroll
        for (int jt = 0; jt < 2; ++jt) {
          if (diagw && !(it == 0 && jt == 1)) continue;
          if (!plain(it, jt)) continue;
#pragma unroll
          for (int r = 0; r < 4; ++r) sM[lo * 17 + 4 * r + hi] = acc[it][jt][r];
          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
          for (int k = 0; k < 4; ++k) pm[(size_t)(16 * jt + 4 * k) * ld + 16 * it] = sM[(4 * k + hi) * 17 + lo];
          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        }
    }
    if (interior) return;
  }
  double* xb = x + (size_t)b * ld;
#pragma unroll
  for (int it = 0; it < 2; ++it)
#pragma unroll
    for (int jt = 0; jt < 2; ++jt) {
      if (plain(it, jt)) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = i0 + 16 * it + hi + 4 * r, col = j0 + 16 * jt + lo;
        const double v = acc[it][jt][r];
        if (col == ld - 1) {
          if (row != ld - 1) xb[row] += v;  // x += V (L^-1 nu)
        } else if (row != ld - 1) {
          const double pn = pold[it][jt][r] - v;
          Pb[(size_t)row * ld + col] = pn;
          if (mirror) Pb[(size_t)col * ld + row] = pn;
        }
      }
    }
}

// P -= V V^T, x += V (L^-1 nu)
int launch_product(sl2_engine* e) {
  const int B = e->B;
  LaunchScope ls(e, "k_syrk", true);
  const int nt = e->ld / 64;
#ifdef SL2_CHOL_TRACE   // the stamp buffer is the Cholesky's unless SL2_TRACE_SYRK is set (scripts/syrk_clock.py sets it)
  static const bool trace_syrk = getenv("SL2_TRACE_SYRK") != nullptr;
  hipLaunchKernelGGL(k_syrk, dim3(xcd_grid(nt * (nt + 1) / 2, B)), dim3(256), 0, e->stream, e->Vt, e->P, e->x, e->m_gate,
                     e->ld, e->mld, B, e->n_slots, e->ppos, trace_syrk ? (long long*)e->root->chol_trace : nullptr);
#else
  hipLaunchKernelGGL(k_syrk, dim3(xcd_grid(nt * (nt + 1) / 2, B)), dim3(256), 0, e->stream, e->Vt, e->P, e->x, e->m_gate,
                     e->ld, e->mld, B, e->n_slots, e->ppos);
#endif
  SL2_HIP(hipGetLastError());
  return SL2_OK;
}

// k_syrk on the given covariance and V^T, everything else the engine's: sl2_create's placement probe (sl2_engine.hip:
// place_large_matrices), which fills m_count / n_slots for the occasion - on an engine that holds nothing but zeros the launch
// does its full work and changes nothing.
int launch_syrk_on(sl2_engine* e, const double* Vt, double* P) {
  const int nt = e->ld / 64;
#ifdef SL2_CHOL_TRACE
  hipLaunchKernelGGL(k_syrk, dim3(xcd_grid(nt * (nt + 1) / 2, e->B)), dim3(256), 0, e->stream, Vt, P, e->x, e->m_count, e->ld, e->mld, e->B,
                     e->n_slots, e->ppos, (long long*)nullptr);
#else
  hipLaunchKernelGGL(k_syrk, dim3(xcd_grid(nt * (nt + 1) / 2, e->B)), dim3(256), 0, e->stream, Vt, P, e->x, e->m_count, e->ld, e->mld, e->B,
                     e->n_slots, e->ppos);
#endif
  SL2_HIP(hipGetLastError());
  return SL2_OK;
}

}  // namespace sl2
