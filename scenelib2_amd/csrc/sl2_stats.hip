// sl2_get_step_stats (include/scenelib2_amd.h): the filter-consistency record of the last completed update for a RANGE of
// sequences in one launch - what sl2_get_selection / sl2_snapshot give one sequence and one synchronisation at a time, plus the
// EKF health figures nothing else exposes (normalised innovation squared, log det S, the pivots of the innovation Cholesky).
//
// Nothing is computed ahead of the question.  Every form of the update leaves, per sequence b with m = 2 m_gate[b] rows,
//   Vt[b][r][ld - 1]       = w_r, w = L^-1 nu      (the innovation rides through the substitution as the last column of A^T:
//                            k_fwdsub_ksplit, k_fwdsub_lds<NB>, the grouped form with k_fwd_gemm - sl2_update_fwdsub.hip; the fused
//                            small-map step stores it from its LDS panel - sl2_small.hip)
//   LinvT[b][r / 32][r % 32][r % 32] = 1 / L_rr    (k_chol_left keeps the diagonal blocks of L in LDS and writes only their
//                            inverses, one launch or panel-wise; St's diagonal blocks still hold S there, so the pivot is taken
//                            from the inverse; k_small_back stores the same word)
// and f_nu / f_S / succ_idx / the per-sequence counters survive until the next step.  k_step_stats reads exactly those.
//
// Order of every floating-point operation (part of the contract: the bytes of a record depend on nothing but the sequence's own
// state): one wavefront per sequence; lane l walks rows l, l + 64, ... in ascending order; the 64 partial results meet in a
// butterfly over lane distances 32, 16, 8, 4, 2, 1.  Sums, min, max and the arg-max over the matched features all go that way.
#include "sl2_common.hpp"

namespace sl2 {

static_assert(sizeof(sl2_step_stats) == 96, "sl2_step_stats is 96 bytes");

constexpr int kStatThreads = 256;      // four sequences per workgroup, a wavefront each

__device__ __forceinline__ double bfly_f64(double v, int dist) { return __shfl_xor(v, dist, 64); }

__global__ void __launch_bounds__(kStatThreads) k_step_stats(const SeqArrays a, int seq0, int nseq, int N, int ld, int mld,
                                                            int nblk_max, sl2_step_stats* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int s = blockIdx.x * (kStatThreads / 64) + (threadIdx.x >> 6);
  if (s >= nseq) return;                               // (a whole wavefront)
  const int b = seq0 + s;
  const size_t o = (size_t)b * N;
  const int status = a.status[b];
  const bool stepped = a.step_mark[b] != 0 && !(status & SL2_STATUS_SMALL_STEP_REFUSED);
  int cnt = stepped ? a.m_gate[b] : 0;
  cnt = cnt < 0 ? 0 : (2 * cnt > mld ? mld / 2 : cnt);  // (cannot happen: m_gate <= nsel_max; nothing is read outside the workspaces)
  const int m = 2 * cnt;

  // ---- the joint system: w and the pivots, rows lane, lane + 64, ...
  const double* wb = a.Vt + (size_t)b * mld * ld + (ld - 1);
  const double* lb = a.LinvT + (size_t)b * nblk_max * 1024;
  double nis = 0.0, logdet = 0.0, pmin = __builtin_inf(), pmax = -__builtin_inf();
  for (int r = lane; r < m; r += 64) {
    const double w = wb[(size_t)r * ld];
    const double linv = lb[(size_t)(r >> 5) * 1024 + (r & 31) * 33];
    const double piv = 1.0 / linv;
    nis = __builtin_fma(w, w, nis);
    logdet += log(piv);                                // a log per pivot: no product that could leave the range
    pmin = piv < pmin ? piv : pmin;
    pmax = piv > pmax ? piv : pmax;
  }
  // ---- the matched features' own distances nu_i^T S_i^-1 nu_i (f_nu, f_S: what sl2_feature_info reports), slot order
  double best = -1.0;
  int best_f = 0x7fffffff;
  for (int j = lane; j < cnt; j += 64) {
    const int f = a.succ_idx[o + j];
    if (f < 0 || f >= N) continue;
    const double n0 = a.f_nu[(o + f) * 2], n1 = a.f_nu[(o + f) * 2 + 1];
    const double s00 = a.f_S[(o + f) * 4], s01 = a.f_S[(o + f) * 4 + 1], s10 = a.f_S[(o + f) * 4 + 2], s11 = a.f_S[(o + f) * 4 + 3];
    const double det = s00 * s11 - s01 * s10;
    const double d2 = (n0 * (s11 * n0 - s01 * n1) + n1 * (s00 * n1 - s10 * n0)) / det;
    if (d2 > best) { best = d2; best_f = f; }          // (ascending slots: a tie stays with the lower one)
  }
  // ---- the counts sl2_snapshot_header reports: feature_list_.size() and the selection without the deleted features
  const int ns = min(max(a.n_slots[b], 0), N), nsel_raw = min(max(a.n_sel[b], 0), N);
  int nfeat = 0, nkept = 0;
  for (int f = lane; f < ns; f += 64) {
    const int fl = a.f_flags[o + f];
    nfeat += ((fl & FF_PARTIAL) || (fl & FF_ACTIVE)) ? 1 : 0;
  }
  for (int k = lane; k < nsel_raw; k += 64) {
    const int f = a.sel_idx[o + k];
    nkept += (f >= 0 && f < ns && (a.f_flags[o + f] & FF_ACTIVE)) ? 1 : 0;
  }
  // ---- the butterfly: after it every lane holds the same values
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    nis += bfly_f64(nis, d);
    logdet += bfly_f64(logdet, d);
    const double qmin = bfly_f64(pmin, d), qmax = bfly_f64(pmax, d);
    pmin = qmin < pmin ? qmin : pmin;
    pmax = qmax > pmax ? qmax : pmax;
    const double qb = bfly_f64(best, d);
    const int qf = __shfl_xor(best_f, d, 64);
    if (qb > best || (qb == best && qf < best_f)) { best = qb; best_f = qf; }
    nfeat += __shfl_xor(nfeat, d, 64);
    nkept += __shfl_xor(nkept, d, 64);
  }
  if (lane != 0) return;
  const double* Pb = a.P + (size_t)b * ld * ld;
  const bool have = best_f != 0x7fffffff;
  sl2_step_stats r;
  r.stepped = stepped ? 1 : 0;
  r.status_flags = status;
  r.sequence_steps = (a.pos_count[b] + a.seq_age[b]) & 0x7fffffff;
  r.n_features = nfeat;
  r.n_partial = a.part_i[(size_t)b * kPartInts + kPartCount];
  r.n_visible = a.n_vis[b];
  r.n_selected = nkept;
  r.n_matched = a.m_count[b];
  r.dof = m;
  r.worst_label = have ? a.f_label[o + best_f] : -1;
  r.nis = nis;
  r.log_det_S = 2.0 * logdet;
  r.min_pivot = m ? pmin : 0.0;
  r.max_pivot = m ? pmax : 0.0;
  r.worst_feature_d2 = have ? best : 0.0;
  r.position_var = (Pb[0] + Pb[(size_t)ld + 1]) + Pb[2 * (size_t)ld + 2];
  r.reserved[0] = 0; r.reserved[1] = 0;
  out[s] = r;
}

}  // namespace sl2

using namespace sl2;

extern "C" int sl2_get_step_stats(sl2_engine* e, int seq0, int nseq, sl2_step_stats* out, int out_on_device) {
  if (!e || seq0 < 0 || nseq <= 0 || seq0 > e->B - nseq || !out || (out_on_device && (uintptr_t)out % 8)) {
    set_error("sl2_get_step_stats: bad argument");
    return SL2_ERR_INVALID;
  }
  SL2_HIP(hipSetDevice(e->device));
  if (!out_on_device && !e->stats_host) {    // first use of the host form: one pinned, mapped buffer for the whole batch
    SL2_HIP(hipHostMalloc(&e->stats_host, sizeof(sl2_step_stats) * (size_t)e->B, hipHostMallocMapped));
    SL2_HIP(hipHostGetDevicePointer(&e->stats_host_dev, e->stats_host, 0));
  }
  // on the engine's stream: the groups' streams (sl2_set_groups > 1) join it at the end of every stepping call, and a replayed
  // graph is one more node in front of this launch.  The root's arrays: a record does not know which group stepped its sequence.
  sl2_step_stats* dst = out_on_device ? out : (sl2_step_stats*)e->stats_host_dev;
  {
    LaunchScope ls(e, "k_step_stats");
    hipLaunchKernelGGL(k_step_stats, dim3((nseq + kStatThreads / 64 - 1) / (kStatThreads / 64)), dim3(kStatThreads), 0, e->stream, seq_arrays(e),
                       seq0, nseq, e->N, e->ld, e->mld, e->nblk_max, dst);
    SL2_HIP(hipGetLastError());
  }
  if (out_on_device) return SL2_OK;
  SL2_HIP(hipStreamSynchronize(e->stream));
  memcpy(out, e->stats_host, sizeof(sl2_step_stats) * (size_t)nseq);
  return SL2_OK;
}
