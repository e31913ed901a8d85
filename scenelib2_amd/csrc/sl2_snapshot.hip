// sl2_snapshot: the one-call read-back of a sequence's public state (include/scenelib2_amd.h).
//
// The reference's callers read the MonoSLAM object's public members after every GoOneStep at zero cost
// (examples/MonoSlamSceneLib1.cpp:132-151; graphic/graphictool.cpp:130-167, 290-347 walk xv_, Pxx_ and every Feature's y_,
// Pxy_, Pyy_, h_, z_, S_, flags).  Here those members live in HBM, spread over the engine's per-slot arrays and the dense
// covariance.  k_snapshot gathers them for ONE sequence into a packed blob in a device staging buffer (per-feature records
// in feature_list_ order, deleted features removed, the Pxy / Pyy blocks cut out of P) and then streams the blob - exactly
// its size, in coalesced 16-byte pieces - into a pinned, mapped host buffer owned by the engine: one launch, one stream
// synchronisation, no hipMemcpy, no allocation per call.
//
// sl2_snapshot_batch is the same read for a RANGE of sequences: the packing is one __device__ function (snapshot_body) that
// k_snapshot calls for its one sequence and k_snapshot_batch for each of its range, behind a sizing launch and a scan that say where
// every blob goes.
#include "sl2_common.hpp"

#include <chrono>

namespace sl2 {

constexpr int kSnapMagic = 0x53324c53;
constexpr int kSnapThreads = 256;
constexpr int kFeatureInfoBytes = (int)sizeof(sl2_feature_info);
static_assert(sizeof(sl2_snapshot_header) == 256, "sl2_snapshot_header is 64 ints");
static_assert(sizeof(sl2_feature_info) % 8 == 0, "feature records keep the sections 8-byte aligned");
static_assert(sizeof(sl2_partial_info) == 32, "sl2_partial_info");

__device__ __forceinline__ int up8(int v) { return (v + 7) & ~7; }

// Which slots are in feature_list_, and as what: the one reading of f_flags that the counting phases below share.
__device__ __forceinline__ bool slot_partial(int fl) { return (fl & FF_PARTIAL) != 0; }
__device__ __forceinline__ bool slot_full(int fl) { return !(fl & FF_PARTIAL) && (fl & FF_ACTIVE) != 0; }

// What the blob of a sequence carries, and where: the ONE place that turns a sequence's counts, the caller's cursor and the
// sections asked for into the offsets and the size of the blob.  k_snapshot_sizes calls it to size a blob and snapshot_body to
// write the header, so the two cannot disagree.  An omitted section has length 0 and its offset is the running one.
struct SnapLayout {
  int off_xv, off_Pxx, off_features, off_cov, off_selection, off_traj, off_partial, off_patches, bytes;
  int traj_first, traj_count, n_patches;
};
__device__ __forceinline__ SnapLayout snapshot_layout(int sections, int nf, int cov_doubles, int kept, int traj_total, int traj_cursor, int n_partial,
                                                      int n_particles, int n_patches) {
  SnapLayout l;
  int first = traj_total - kTrajCapacity;
  if (first < 0) first = 0;
  if (first < traj_cursor) first = traj_cursor;      // (a negative cursor is 0: first >= 0 already)
  if (first > traj_total) first = traj_total;
  if (!(sections & SL2_SNAP_TRAJ)) first = traj_total;
  l.traj_first = first; l.traj_count = traj_total - first;
  l.n_patches = (sections & SL2_SNAP_PATCHES) ? n_patches : 0;
  int off = (int)sizeof(sl2_snapshot_header);
  l.off_xv = off; off += 13 * 8;
  l.off_Pxx = off; off += 169 * 8;
  l.off_features = off; if (sections & SL2_SNAP_FEATURES) off += nf * kFeatureInfoBytes;
  l.off_cov = off; if (sections & SL2_SNAP_COV) off += cov_doubles * 8;
  l.off_selection = off; if (sections & SL2_SNAP_SELECTION) off += up8(kept * 4);
  l.off_traj = off; off += l.traj_count * 24;
  l.off_partial = off; if (sections & SL2_SNAP_PARTIAL) off += n_partial * (int)sizeof(sl2_partial_info) + n_particles * kParticleDoubles * 8;
  l.off_patches = off; off += l.n_patches * 128;
  l.bytes = off;
  return l;
}

// The blob of ONE sequence, written by one workgroup straight to dst (device memory, 16-byte aligned): what k_snapshot packs for
// its one sequence and k_snapshot_batch for each of its range.  With SL2_SNAP_ALL the bytes are sl2_snapshot's.
// LDS (sm, 8 N ints): per slot flags, label, list index (-1: not in feature_list_), state size, first double of its
// covariance record, patch index (-1: not included); then the selection's labels.
// `room` = the bytes dst has for it: a blob that would not fit is not written at all and the call returns true (the whole
// workgroup alike; k_snapshot's staging holds sl2_snapshot_capacity and passes no limit).
__device__ __forceinline__ bool snapshot_body(const SeqArrays& a, int seq, unsigned char* __restrict__ stage, int sections, int traj_cursor,
                                              int patch_from_label, int N, int ld, int ppos, int pcap, int kpart, long long steps_done, int* sm,
                                              sl2_snapshot_header& hd, unsigned long long room) {
  int* s_flags = sm;
  int* s_label = sm + N;
  int* s_li = sm + 2 * N;
  int* s_cov = sm + 3 * N;
  int* s_pi = sm + 4 * N;
  int* s_pos = sm + 5 * N;
  int* s_sel = sm + 6 * N;
  int* s_col = sm + 7 * N;                     // first state column of a live slot's feature
  const int tid = threadIdx.x;
  const size_t o = (size_t)seq * N;
  const int ns = min(max(a.n_slots[seq], 0), N);      // (never outside: the LDS above is laid out for N slots)
  const int nsel_raw = min(max(a.n_sel[seq], 0), N);
  const int* pi = a.part_i + (size_t)seq * kPartInts;
  const int* psb = a.ps_i + (size_t)seq * kpart * kPsInts;
  __shared__ int s_ps[kMaxPartial][kPsInts];
  if (tid < kpart * kPsInts) s_ps[tid / kPsInts][tid % kPsInts] = psb[tid];
  // the partial slot whose label sits in feature slot f (-1: none)
  auto pslot_of = [&](int f) { int r = -1; for (int k = 0; k < kpart; ++k) if (s_ps[k][kPsActive] && s_ps[k][kPsLabel] == f) r = k; return r; };
  for (int f = tid; f < ns; f += kSnapThreads) { s_flags[f] = a.f_flags[o + f]; s_label[f] = a.f_label[o + f]; }
  for (int k = tid; k < nsel_raw; k += kSnapThreads) s_sel[k] = a.sel_idx[o + k];
  __syncthreads();
  // list positions, state positions, covariance offsets and the compacted selection: one wavefront, ballots and popcounts
  // (a single thread walking the slots through LDS was 15 us of a 40 us kernel at 100 features)
  __shared__ int s_tot[5];                     // nf, total state size, covariance doubles, patches, kept selection entries
  if (tid < 64) {
    int nfull = 0, npart = 0, npatch = 0;      // running counts in front of the current 64 slots (wave-uniform)
    for (int base = 0; base < ns; base += 64) {
      const int f = base + tid;
      const int fl = f < ns ? s_flags[f] : 0;
      const bool part = slot_partial(fl), full = slot_full(fl);
      const bool wants_patch = (part || full) && s_label[f < ns ? f : 0] >= patch_from_label;
      const unsigned long long m_full = __ballot(full), m_part = __ballot(part), m_pat = __ballot(wants_patch);
      const unsigned long long below = (1ull << tid) - 1ull;
      const int cf = nfull + __popcll(m_full & below), cp = npart + __popcll(m_part & below);
      if (f < ns) {
        s_li[f] = (part || full) ? cf + cp : -1;
        s_pos[f] = 13 + 3 * cf + 6 * cp;
        s_cov[f] = (13 * 3 + 9) * cf + (13 * 6 + 36) * cp;
        s_pi[f] = wants_patch ? npatch + __popcll(m_pat & below) : -1;
      }
      nfull += __popcll(m_full); npart += __popcll(m_part); npatch += __popcll(m_pat);
    }
    // delete_feature() deselects the feature it removes (monoslam.cpp:800-801)
    int kept = 0;
    for (int base = 0; base < nsel_raw; base += 64) {
      const int k = base + tid;
      const int f = k < nsel_raw ? s_sel[k] : -1;
      const bool ok = f >= 0 && f < ns && (s_flags[f] & FF_ACTIVE);
      const int lab = ok ? s_label[f] : 0;
      const unsigned long long m = __ballot(ok);
      if (ok) s_sel[kept + __popcll(m & ((1ull << tid) - 1ull))] = lab;      // (destinations lie at or below this round's sources)
      kept += __popcll(m);
    }
    if (tid == 0) { s_tot[0] = nfull + npart; s_tot[1] = 13 + 3 * nfull + 6 * npart; s_tot[2] = 48 * nfull + 114 * npart; s_tot[3] = npatch; s_tot[4] = kept; }
  }
  __syncthreads();
  if (tid == 0) {
    const int nf = s_tot[0], pos = s_tot[1], cov = s_tot[2], np = s_tot[3], kept = s_tot[4];
    const int total = a.traj_count[seq];
    const int n_partial = pi[kPartCount];
    int n_particles = 0;                       // of all entries of feature_init_info_vector_ together
    for (int q = 0; q < n_partial; ++q) n_particles += s_ps[pi[kPartOrder + q]][kPsNp];
    const SnapLayout l = snapshot_layout(sections, nf, cov, kept, total, traj_cursor, n_partial, n_particles, np);
    int* h = reinterpret_cast<int*>(&hd);
    for (int k = 0; k < 64; ++k) h[k] = 0;
    hd.magic = kSnapMagic; hd.api_version = SL2_API_VERSION; hd.seq = seq;
    hd.n_features = nf; hd.total_state_size = pos;
    hd.number_of_visible_features = a.n_vis[seq];
    hd.n_selected = kept;
    hd.successful_measurement_vector_size = 2 * a.m_count[seq];
    hd.next_free_label = a.next_label[seq];
    hd.status_flags = a.status[seq];
    hd.traj_total = total; hd.traj_first = l.traj_first; hd.traj_count = l.traj_count;
    hd.n_partial = n_partial; hd.n_patches = l.n_patches;
    hd.uu = pi[kPartUU]; hd.vv = pi[kPartVV];
    hd.location_selected_flag = pi[kPartCreated];
    hd.init_feature_search_region_defined_flag = pi[kPartRegionValid];
    for (int k = 0; k < 4; ++k) hd.init_feature_search_region[k] = pi[kPartRegion + k];
    hd.steps_done = (int)(steps_done & 0x7fffffff);
    hd.sequence_steps = (a.pos_count[seq] + a.seq_age[seq]) & 0x7fffffff;
    hd.omitted_sections = SL2_SNAP_ALL & ~sections;
    hd.off_xv = l.off_xv; hd.off_Pxx = l.off_Pxx; hd.off_features = l.off_features; hd.off_cov = l.off_cov;
    hd.off_selection = l.off_selection; hd.off_traj = l.off_traj; hd.off_partial = l.off_partial; hd.off_patches = l.off_patches;
    hd.bytes = l.bytes;
  }
  __syncthreads();
  if ((((unsigned long long)hd.bytes + 15ull) & ~15ull) > room) return true;
  const bool with_features = (sections & SL2_SNAP_FEATURES) != 0, with_cov = with_features && (sections & SL2_SNAP_COV) != 0;
  const double* xb = a.x + (size_t)seq * ld;
  const double* Pb = a.P + (size_t)seq * ld * ld;
  // header, xv_, Pxx_
  for (int k = tid; k < 64; k += kSnapThreads) reinterpret_cast<int*>(stage)[k] = reinterpret_cast<const int*>(&hd)[k];
  double* o_xv = reinterpret_cast<double*>(stage + hd.off_xv);
  double* o_Pxx = reinterpret_cast<double*>(stage + hd.off_Pxx);
  for (int k = tid; k < 13; k += kSnapThreads) o_xv[k] = xb[k];
  for (int k = tid; k < 169; k += kSnapThreads) o_Pxx[k] = Pb[(size_t)(k / 13) * ld + (k % 13)];
  // feature records + covariance blocks
  for (int f = tid; f < (with_features ? ns : 0); f += kSnapThreads) {
    const int li = s_li[f];
    if (li < 0) continue;
    const int fl = s_flags[f];
    const bool partial = (fl & FF_PARTIAL) != 0;
    const int d = partial ? 6 : 3;
    const int col = partial ? ppos + 6 * (pslot_of(f) < 0 ? 0 : pslot_of(f)) : 13 + 3 * f;
    sl2_feature_info fi;
    fi.label = s_label[f];
    fi.active = 1;
    fi.selected_flag = (fl & FF_SELECTED) ? 1 : 0;
    fi.successful_measurement_flag = (fl & FF_SUCCESS) ? 1 : 0;
    fi.attempted_measurements_of_feature = a.attempted[o + f];
    fi.successful_measurements_of_feature = a.successful[o + f];
    fi.position_in_total_state_vector = s_pos[f] - a.pos_err[o + f];      // (Q28: what the reference has on record)
    fi.visible = (fl & FF_VISIBLE) ? 1 : 0;
    for (int k = 0; k < 3; ++k) fi.y[k] = xb[col + k];
    for (int k = 0; k < 2; ++k) { fi.h[k] = a.f_h[(o + f) * 2 + k]; fi.z[k] = a.f_z[(o + f) * 2 + k]; fi.nu[k] = a.f_nu[(o + f) * 2 + k]; }
    fi.R = a.f_R[o + f];
    for (int k = 0; k < 4; ++k) fi.S[k] = a.f_S[(o + f) * 4 + k];
    for (int k = 0; k < 14; ++k) fi.dh_by_dxp[k] = a.f_Hx[(o + f) * 14 + k];
    for (int k = 0; k < 6; ++k) fi.dh_by_dy[k] = a.f_Hy[(o + f) * 6 + k];
    for (int k = 0; k < 7; ++k) fi.xp_org[k] = a.xp_org[(o + f) * 8 + k];
    fi.fully_initialised_flag = partial ? 0 : 1;
    fi.state_size = d;
    for (int k = 0; k < 3; ++k) fi.y_direction[k] = partial ? xb[col + 3 + k] : 0.0;
    *reinterpret_cast<sl2_feature_info*>(stage + hd.off_features + (size_t)li * kFeatureInfoBytes) = fi;
    s_col[f] = col;
  }
  __syncthreads();
  // Pxy_ / Pyy_ blocks and the new templates: one (feature, element) pair per thread and round, so that the ~50 loads of a
  // feature's blocks are spread over lanes instead of queued on one
  for (int idx = tid; idx < (with_cov ? ns * 128 : 0); idx += kSnapThreads) {
    const int f = idx >> 7, el = idx & 127;
    if (s_li[f] < 0) continue;
    const int d = (s_flags[f] & FF_PARTIAL) ? 6 : 3, col = s_col[f];
    if (el >= 13 * d + d * d) continue;
    double* oc = reinterpret_cast<double*>(stage + hd.off_cov) + s_cov[f];
    if (el < 13 * d) oc[el] = Pb[(size_t)(el / d) * ld + col + el % d];
    else { const int q = el - 13 * d; oc[el] = Pb[(size_t)(col + q / d) * ld + col + q % d]; }
  }
  if (hd.n_patches)
    for (int idx = tid; idx < ns * 128; idx += kSnapThreads) {
      const int f = idx >> 7, el = idx & 127;
      const int pidx = s_li[f] >= 0 ? s_pi[f] : -1;
      if (pidx < 0) continue;
      unsigned char* op = stage + hd.off_patches + (size_t)pidx * 128;
      if (el < 4) op[el] = (unsigned char)((unsigned)s_label[f] >> (8 * el));            // int32 label, little endian
      else if (el < 4 + SL2_PATCH_BYTES) op[el] = a.patch[(o + f) * kPatchStride + el - 4];
      else op[el] = 0;
    }
  // selected_feature_list_ as labels
  int* o_sel = reinterpret_cast<int*>(stage + hd.off_selection);
  const int n_sel_out = (sections & SL2_SNAP_SELECTION) ? hd.n_selected : 0;
  for (int k = tid; k < n_sel_out; k += kSnapThreads) o_sel[k] = s_sel[k];
  if (tid == 0 && (n_sel_out & 1)) o_sel[n_sel_out] = 0;
  // trajectory_store_: the entries the caller has not seen yet
  double* o_tr = reinterpret_cast<double*>(stage + hd.off_traj);
  for (int k = tid; k < hd.traj_count * 3; k += kSnapThreads) {
    const int logical = hd.traj_first + k / 3;
    o_tr[k] = a.traj[((size_t)seq * kTrajCapacity + (logical % kTrajCapacity)) * 3 + (k % 3)];
  }
  // feature_init_info_vector_, in the vector's order
  {
    unsigned char* out = stage + hd.off_partial;
    for (int q = 0; q < ((sections & SL2_SNAP_PARTIAL) ? hd.n_partial : 0); ++q) {
      const int ks = pi[kPartOrder + q];
      const int npart = s_ps[ks][kPsNp];
      sl2_partial_info* pinfo = reinterpret_cast<sl2_partial_info*>(out);
      if (tid == 0) {
        const int slot = s_ps[ks][kPsLabel];
        pinfo->label = (slot >= 0 && slot < ns) ? s_label[slot] : -1;
        pinfo->number_of_match_attempts = s_ps[ks][kPsAttempts];
        pinfo->n_particles = npart;
        pinfo->making_measurement_on_this_step_flag = s_ps[ks][kPsMaking];
        pinfo->mean = a.ps_d[((size_t)seq * kpart + ks) * kPsDoubles + 0];
        pinfo->covariance = a.ps_d[((size_t)seq * kpart + ks) * kPsDoubles + 1];
      }
      double* opp = reinterpret_cast<double*>(pinfo + 1);
      const double* src = a.particles + ((size_t)seq * kpart + ks) * pcap * kParticleDoubles;
      for (int k = tid; k < npart * kParticleDoubles; k += kSnapThreads) opp[k] = src[k];
      out += sizeof(sl2_partial_info) + (size_t)npart * kParticleDoubles * 8;
    }
  }
  return false;
}

// sl2_snapshot: one workgroup packs the sequence's blob into the staging buffer and streams it to the host.
__global__ void __launch_bounds__(kSnapThreads) k_snapshot(const SeqArrays a, int seq, int N, int ld, int ppos, int pcap, int kpart, int traj_cursor,
                                                           int patch_from_label, long long steps_done, unsigned char* __restrict__ stage,
                                                           uint4* __restrict__ host_out, unsigned long long* __restrict__ done_word,
                                                           unsigned long long ticket) {
  extern __shared__ int sm[];
  __shared__ sl2_snapshot_header hd;
  const int tid = threadIdx.x;
  snapshot_body(a, seq, stage, SL2_SNAP_ALL, traj_cursor, patch_from_label, N, ld, ppos, pcap, kpart, steps_done, sm, hd, ~0ull);
  // the blob leaves for the host: the workgroup's own stores above are visible to it after the barrier
  __threadfence();
  __syncthreads();
  const int n16 = (hd.bytes + 15) >> 4;
  const uint4* src16 = reinterpret_cast<const uint4*>(stage);
  for (int k = tid; k < n16; k += kSnapThreads) host_out[k] = src16[k];
  __threadfence_system();
  // The blob is in host memory: say so in a word of its own, so that the caller can pick it up the moment it is complete instead
  // of waiting for the launch to be retired (sl2_snapshot spins on this word first: ~8 us less per call than a stream wait).
  __syncthreads();
  if (tid == 0) __hip_atomic_store(done_word, ticket, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// ---- sl2_snapshot_batch: the blobs of a RANGE of sequences, packed back to back, in three launches on the engine's stream.
// Each launch depends on the one before it and on nothing inside itself: no workgroup reads what another of the same launch
// writes, so there is no look-back, no last arriver and no wait - the stream is the only order.
constexpr int kSizeSeqs = kSnapThreads / 64;      // sequences per workgroup of k_snapshot_sizes, a wavefront each
constexpr int kScanChunk = 256;                   // sizes per round of k_snapshot_scan

__device__ __forceinline__ void load_cursor(const int32_t* __restrict__ cursors, int i, int* traj_cursor, int* patch_from_label) {
  *traj_cursor = cursors ? cursors[2 * i] : 0;
  *patch_from_label = cursors ? cursors[2 * i + 1] : 0;
  if (*traj_cursor < 0) *traj_cursor = 0;
}

// 1. sizes[i] = header.bytes of the blob of sequence seq0 + i: the counts of snapshot_body's counting phase without its tables.
__global__ void __launch_bounds__(kSnapThreads) k_snapshot_sizes(const SeqArrays a, int seq0, int nseq, int N, int kpart, int sections,
                                                                 const int32_t* __restrict__ cursors, unsigned long long* __restrict__ sizes) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * kSizeSeqs + (threadIdx.x >> 6);
  if (i >= nseq) return;                               // (a whole wavefront)
  const int seq = seq0 + i;
  const size_t o = (size_t)seq * N;
  int traj_cursor, patch_from_label;
  load_cursor(cursors, i, &traj_cursor, &patch_from_label);
  const int ns = min(max(a.n_slots[seq], 0), N), nsel_raw = min(max(a.n_sel[seq], 0), N);
  int nfull = 0, npart = 0, npatch = 0, kept = 0;      // wave-uniform
  for (int base = 0; base < ns; base += 64) {
    const int f = base + lane;
    const int fl = f < ns ? a.f_flags[o + f] : 0;
    const bool part = slot_partial(fl), full = slot_full(fl);
    const bool wants_patch = (part || full) && a.f_label[o + (f < ns ? f : 0)] >= patch_from_label;
    nfull += __popcll(__ballot(full)); npart += __popcll(__ballot(part)); npatch += __popcll(__ballot(wants_patch));
  }
  for (int base = 0; base < nsel_raw; base += 64) {
    const int k = base + lane;
    const int f = k < nsel_raw ? a.sel_idx[o + k] : -1;
    const bool ok = f >= 0 && f < ns && (a.f_flags[o + (f >= 0 && f < ns ? f : 0)] & FF_ACTIVE);
    kept += __popcll(__ballot(ok));
  }
  if (lane != 0) return;
  const int* pi = a.part_i + (size_t)seq * kPartInts;
  const int* psb = a.ps_i + (size_t)seq * kpart * kPsInts;
  const int n_partial = pi[kPartCount];
  int n_particles = 0;
  for (int q = 0; q < n_partial; ++q) {
    const int ks = pi[kPartOrder + q];
    if (ks >= 0 && ks < kpart) n_particles += psb[ks * kPsInts + kPsNp];
  }
  const SnapLayout l = snapshot_layout(sections, nfull + npart, 48 * nfull + 114 * npart, kept, a.traj_count[seq], traj_cursor, n_partial, n_particles, npatch);
  sizes[i] = (unsigned long long)l.bytes;
}

// 2. offsets[0 .. nseq] = the exclusive scan of the sizes rounded up to 16, in place (the sizes arrive in offsets[0 .. nseq - 1]).
// One workgroup walks the range in chunks with a carry, so that any batch size works; every thread holds its chunk's value in a
// register across the barriers, so that overwriting the chunk is safe.
__global__ void __launch_bounds__(kScanChunk) k_snapshot_scan(unsigned long long* __restrict__ offsets, int nseq) {
  __shared__ unsigned long long s[kScanChunk];
  const int tid = threadIdx.x;
  unsigned long long carry = 0;
  for (int base = 0; base < nseq; base += kScanChunk) {
    const int i = base + tid;
    const unsigned long long v = i < nseq ? (offsets[i] + 15ull) & ~15ull : 0ull;
    s[tid] = v;
    __syncthreads();
    for (int d = 1; d < kScanChunk; d <<= 1) {
      const unsigned long long t = tid >= d ? s[tid - d] : 0ull;
      __syncthreads();
      s[tid] += t;
      __syncthreads();
    }
    if (i < nseq) offsets[i] = carry + s[tid] - v;
    carry += s[kScanChunk - 1];
    __syncthreads();
  }
  if (tid == 0) offsets[nseq] = carry;
}

// 3. one workgroup per sequence writes its blob at out + offsets[i].  Nothing is written when the blobs do not fit (the caller
// reads the size it needs from offsets[nseq]), and a blob whose size is not the one its place was cut for is not written either
// (cannot happen: both kernels take it from snapshot_layout on the same state; nothing is ever stored outside the blob's place).
__global__ void __launch_bounds__(kSnapThreads) k_snapshot_batch(const SeqArrays a, int seq0, int N, int ld, int ppos, int pcap, int kpart, int sections,
                                                                 const int32_t* __restrict__ cursors, long long steps_done,
                                                                 unsigned char* __restrict__ out, unsigned long long out_bytes,
                                                                 const unsigned long long* __restrict__ offsets, int nseq) {
  extern __shared__ int sm[];
  __shared__ sl2_snapshot_header hd;
  if (offsets[nseq] > out_bytes) return;               // (the whole grid)
  const int i = blockIdx.x, tid = threadIdx.x;
  const unsigned long long at = offsets[i], room = offsets[i + 1] - at;
  int traj_cursor, patch_from_label;
  load_cursor(cursors, i, &traj_cursor, &patch_from_label);
  unsigned char* dst = out + at;
  if (snapshot_body(a, seq0 + i, dst, sections, traj_cursor, patch_from_label, N, ld, ppos, pcap, kpart, steps_done, sm, hd, room)) return;
  // the bytes up to the next blob are zero (a blob is a multiple of 8 bytes long)
  if (tid == 0 && ((unsigned long long)hd.bytes & 15ull)) *reinterpret_cast<unsigned long long*>(dst + hd.bytes) = 0ull;
}

}  // namespace sl2

using namespace sl2;

extern "C" size_t sl2_snapshot_bound(int max_features, int partial_slots, int particle_capacity, int sections) {
  if (max_features < 0 || partial_slots < 0 || particle_capacity < 0 || (sections & ~SL2_SNAP_ALL)) return 0;
  const size_t N = (size_t)max_features, kpart = (size_t)partial_slots, pcap = (size_t)particle_capacity;
  size_t b = sizeof(sl2_snapshot_header) + 13 * 8 + 169 * 8;
  if (sections & SL2_SNAP_FEATURES) b += N * sizeof(sl2_feature_info);
  if (sections & SL2_SNAP_COV) b += (N * (13 * 3 + 9) + kpart * (13 * 6 + 36)) * 8;
  if (sections & SL2_SNAP_SELECTION) b += (N * 4 + 7) & ~(size_t)7;
  if (sections & SL2_SNAP_TRAJ) b += (size_t)kTrajCapacity * 24;
  if (sections & SL2_SNAP_PARTIAL) b += kpart * (sizeof(sl2_partial_info) + pcap * kParticleDoubles * 8);
  if (sections & SL2_SNAP_PATCHES) b += N * 128;
  return (b + 15) & ~(size_t)15;
}

extern "C" size_t sl2_snapshot_capacity(const sl2_engine* e) {
  if (!e) return 0;
  return sl2_snapshot_bound(e->N, e->kpart, e->pcap, SL2_SNAP_ALL);
}

// The three launches of sl2_snapshot_batch on the engine's stream.  (The groups' streams - sl2_set_groups > 1 - join it at the end of
// every stepping call, and a replayed graph is one more node in front of them.  The root's arrays: a blob does not know which group
// stepped its sequence.)
static int launch_snapshot_batch(sl2_engine* e, int seq0, int nseq, int sections, const int32_t* d_cursors, void* d_out, size_t out_bytes,
                                 unsigned long long* d_offsets) {
  {
    LaunchScope ls(e, "k_snapshot_sizes");
    hipLaunchKernelGGL(k_snapshot_sizes, dim3((nseq + kSizeSeqs - 1) / kSizeSeqs), dim3(kSnapThreads), 0, e->stream, seq_arrays(e), seq0, nseq, e->N,
                       e->kpart, sections, d_cursors, d_offsets);
    SL2_HIP(hipGetLastError());
  }
  {
    LaunchScope ls(e, "k_snapshot_scan");
    hipLaunchKernelGGL(k_snapshot_scan, dim3(1), dim3(kScanChunk), 0, e->stream, d_offsets, nseq);
    SL2_HIP(hipGetLastError());
  }
  {
    LaunchScope ls(e, "k_snapshot_batch");
    hipLaunchKernelGGL(k_snapshot_batch, dim3(nseq), dim3(kSnapThreads), sizeof(int) * 8 * e->N, e->stream, seq_arrays(e), seq0, e->N, e->ld, e->ppos,
                       e->pcap, e->kpart, sections, d_cursors, e->steps_done, (unsigned char*)d_out, (unsigned long long)out_bytes, d_offsets, nseq);
    SL2_HIP(hipGetLastError());
  }
  return SL2_OK;
}

extern "C" int sl2_snapshot_batch(sl2_engine* e, int seq0, int nseq, int sections, const int32_t* cursors, void* out, size_t out_bytes,
                                  uint64_t* offsets, int on_device) {
  static_assert(sizeof(uint64_t) == sizeof(unsigned long long), "offsets");
  if (!e || !out || !offsets || seq0 < 0 || nseq < 1 || seq0 > e->B - nseq || (sections & ~SL2_SNAP_ALL) ||
      ((sections & SL2_SNAP_COV) && !(sections & SL2_SNAP_FEATURES)) || (on_device && (uintptr_t)out % 16)) {
    set_error("sl2_snapshot_batch: bad argument");
    return SL2_ERR_INVALID;
  }
  if (!on_device && cursors)
    for (int i = 0; i < nseq; ++i)
      if (cursors[2 * i] < 0) { set_error("sl2_snapshot_batch: negative traj_cursor"); return SL2_ERR_INVALID; }
  SL2_HIP(hipSetDevice(e->device));
  if (on_device) return launch_snapshot_batch(e, seq0, nseq, sections, cursors, out, out_bytes, (unsigned long long*)offsets);

  // ---- host form: engine-owned staging (every call below waits before it returns, so one set of buffers serves them all)
  const size_t off_bytes = sizeof(uint64_t) * ((size_t)e->B + 1), aux_bytes = off_bytes + sizeof(int32_t) * 2 * (size_t)e->B;
  if (!e->snapb_aux) {
    SL2_HIP(hipMalloc(&e->snapb_aux, aux_bytes));
    SL2_HIP(hipHostMalloc(&e->snapb_aux_host, aux_bytes, hipHostMallocDefault));
  }
  const size_t need = sl2_snapshot_bound(e->N, e->kpart, e->pcap, sections) * (size_t)nseq;      // no range of blobs is larger
  if (need > e->snapb_stage_bytes) {
    if (e->snapb_stage) { SL2_HIP(hipFree(e->snapb_stage)); e->snapb_stage = nullptr; e->snapb_stage_bytes = 0; }
    SL2_HIP(hipMalloc(&e->snapb_stage, need));
    e->snapb_stage_bytes = need;
  }
  unsigned long long* d_off = (unsigned long long*)e->snapb_aux;
  int32_t* d_cur = nullptr;
  if (cursors) {
    d_cur = (int32_t*)((char*)e->snapb_aux + off_bytes);
    int32_t* h_cur = (int32_t*)((char*)e->snapb_aux_host + off_bytes);
    memcpy(h_cur, cursors, sizeof(int32_t) * 2 * (size_t)nseq);
    SL2_HIP(hipMemcpyAsync(d_cur, h_cur, sizeof(int32_t) * 2 * (size_t)nseq, hipMemcpyHostToDevice, e->stream));
  }
  { int _rc = launch_snapshot_batch(e, seq0, nseq, sections, d_cur, e->snapb_stage, e->snapb_stage_bytes, d_off); if (_rc != SL2_OK) return _rc; }
  // the offset table first: a small copy and the call's one wait ...
  SL2_HIP(hipMemcpyAsync(e->snapb_aux_host, d_off, sizeof(uint64_t) * ((size_t)nseq + 1), hipMemcpyDeviceToHost, e->stream));
  SL2_HIP(hipStreamSynchronize(e->stream));
  memcpy(offsets, e->snapb_aux_host, sizeof(uint64_t) * ((size_t)nseq + 1));
  const uint64_t total = offsets[nseq];
  if (total > e->snapb_stage_bytes) { set_error("sl2_snapshot_batch: malformed offsets"); return SL2_ERR_HIP; }
  if (total > out_bytes) {
    set_error("sl2_snapshot_batch: the blobs need more room than out_bytes (offsets[nseq] has the size)");
    return SL2_ERR_CAPACITY;
  }
  // ... then exactly the packed bytes, in one copy
  SL2_HIP(hipMemcpyAsync(out, e->snapb_stage, (size_t)total, hipMemcpyDeviceToHost, e->stream));
  SL2_HIP(hipStreamSynchronize(e->stream));
  return SL2_OK;
}

extern "C" int sl2_snapshot(sl2_engine* e, int seq, int traj_cursor, int patch_from_label, const void** blob, size_t* bytes) {
  if (!e || seq < 0 || seq >= e->B || !blob || !bytes || traj_cursor < 0) return SL2_ERR_INVALID;
  SL2_HIP(hipSetDevice(e->device));
  if (!e->snap_host) {   // first use: a device staging buffer and a pinned, mapped host buffer, both owned by the engine
    const size_t cap = sl2_snapshot_capacity(e);
    SL2_HIP(hipMalloc(&e->snap_stage, cap));
    // (+ 64 bytes: the completion word behind the blob, on a cache line of its own)
    SL2_HIP(hipHostMalloc(&e->snap_host, cap + 64, hipHostMallocMapped | hipHostMallocCoherent));
    SL2_HIP(hipHostGetDevicePointer(&e->snap_host_dev, e->snap_host, 0));
    e->snap_cap = cap;
    *(volatile unsigned long long*)((char*)e->snap_host + cap) = 0ull;
  }
  // the groups' streams (sl2_set_groups > 1) join the root stream at the end of every stepping call; the kernel below is
  // queued behind them
  hipLaunchKernelGGL(k_snapshot, dim3(1), dim3(kSnapThreads), sizeof(int) * 8 * e->N, e->stream, seq_arrays(e), seq, e->N, e->ld, e->ppos, e->pcap,
                     e->kpart, traj_cursor, patch_from_label, e->steps_done, (unsigned char*)e->snap_stage, (uint4*)e->snap_host_dev,
                     (unsigned long long*)((char*)e->snap_host_dev + e->snap_cap), ++e->snap_ticket);
  SL2_HIP(hipGetLastError());
  {
    // the kernel announces the finished blob in the word behind it; a short spin on that word, then the ordinary wait (a long
    // step in front of the snapshot, a large batch: no point in burning a core)
    const volatile unsigned long long* done = (const volatile unsigned long long*)((const char*)e->snap_host + e->snap_cap);
    const auto t0 = std::chrono::steady_clock::now();
    bool seen = false;
    for (;;) {
      for (int i = 0; i < 64 && !seen; ++i) { seen = __atomic_load_n(done, __ATOMIC_ACQUIRE) == e->snap_ticket; if (!seen) __builtin_ia32_pause(); }
      if (seen || std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(300)) break;
    }
    if (!seen) SL2_HIP(hipStreamSynchronize(e->stream));
  }
  const sl2_snapshot_header* h = (const sl2_snapshot_header*)e->snap_host;
  if (h->magic != kSnapMagic || h->bytes <= 0 || (size_t)h->bytes > sl2_snapshot_capacity(e)) {
    set_error("sl2_snapshot: malformed blob");
    return SL2_ERR_HIP;
  }
  *blob = e->snap_host;
  *bytes = (size_t)h->bytes;
  return SL2_OK;
}
