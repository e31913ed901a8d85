// Engine object, state access and step orchestration behind the C ABI
// (include/scenelib2_amd.h).  Host side of MonoSLAM::GoOneStep
// (monoslam.cpp:108-180): a fixed sequence of batch-wide kernel launches on one
// HIP stream, no host synchronisation inside a step.
#include "sl2_common.hpp"
#include "sl2_mapmath.hpp"

#include <mutex>

namespace sl2 {

static thread_local std::string g_err;
void set_error(const std::string& s) { g_err = s; }

// ------------------------------------------------------------------ small kernels

__global__ void k_add_features(double* __restrict__ x, double* __restrict__ xp_org, uint8_t* __restrict__ patch,
                               int* __restrict__ patch_sums, int* __restrict__ f_flags, int* __restrict__ n_slots,
                               int* __restrict__ attempted, int* __restrict__ successful, int* __restrict__ f_label,
                               int* __restrict__ next_label, const double* __restrict__ y_in,
                               const double* __restrict__ xp_in, const uint8_t* __restrict__ patch_in, int seq0, int nfeat,
                               int N, int ld) {
  // one block per sequence, threads over features
  const int s = blockIdx.x, b = seq0 + s;
  const int base = n_slots[b];
  const int base_label = next_label[b];
  for (int f = threadIdx.x; f < nfeat; f += blockDim.x) {
    const int slot = base + f;
    const size_t fi = (size_t)b * N + slot;
    const size_t src = (size_t)s * nfeat + f;
    for (int k = 0; k < 3; ++k) x[(size_t)b * ld + 13 + 3 * slot + k] = y_in[src * 3 + k];
    for (int k = 0; k < 7; ++k) xp_org[fi * 8 + k] = xp_in[src * 7 + k];
    xp_org[fi * 8 + 7] = 0.0;
    int s0 = 0, s0sq = 0;
    for (int p = 0; p < 121; ++p) {
      const int g = patch_in[src * 121 + p];
      patch[fi * kPatchStride + p] = (uint8_t)g;
      s0 += g; s0sq += g * g;
    }
    for (int p = 121; p < kPatchPackedOffset; ++p) patch[fi * kPatchStride + p] = 0;
    unsigned* packed = (unsigned*)(patch + fi * kPatchStride + kPatchPackedOffset);
    for (int r = 0; r < 11; ++r)
      for (int d = 0; d < 3; ++d) {
        unsigned v = 0;
        for (int k = 0; k < 4; ++k) {
          const int col = 4 * d + k;
          if (col < 11) v |= (unsigned)patch_in[src * 121 + r * 11 + col] << (8 * k);
        }
        packed[r * 3 + d] = v;
      }
    {  // patch sigma test exactly as correlate2_warning + elliptical_search evaluate it (improc.cpp:99-112)
      const double g0bar = (double)s0 / 121.0;
      const double varg0 = (double)s0sq / 121.0 - (g0bar * g0bar);
      const double sigmag0 = sqrt(varg0);
      packed[33] = (unsigned)s0; packed[34] = (unsigned)s0sq;
      packed[35] = (sigmag0 < kCorrelationSigmaThreshold) ? 0u : 1u;
      for (int k = 36; k < (kPatchStride - kPatchPackedOffset) / 4; ++k) packed[k] = 0u;
    }
    patch_sums[fi * 2] = s0; patch_sums[fi * 2 + 1] = s0sq;
    f_flags[fi] = FF_ACTIVE | FF_USED;
    attempted[fi] = 0; successful[fi] = 0;
    f_label[fi] = base_label + f;                 // label_ = next_free_label_++ (monoslam.cpp:1306-1307)
  }
  __syncthreads();
  if (threadIdx.x == 0) { n_slots[b] = base + nfeat; next_label[b] = base_label + nfeat; }
}

__global__ void k_set_feature_cov(double* __restrict__ P, const double* __restrict__ Pyy, int seq0, int nfeat, int ld) {
  const int s = blockIdx.x, b = seq0 + s;
  for (int e = threadIdx.x; e < nfeat * 9; e += blockDim.x) {
    const int f = e / 9, r = (e % 9) / 3, c = e % 3;
    P[(size_t)b * ld * ld + (size_t)(13 + 3 * f + r) * ld + 13 + 3 * f + c] = Pyy[((size_t)s * nfeat + f) * 9 + r * 3 + c];
  }
}

__global__ void k_set_vehicle(double* __restrict__ x, double* __restrict__ P, const double* __restrict__ xv,
                              const double* __restrict__ Pxx, int seq0, int ld) {
  const int s = blockIdx.x, b = seq0 + s;
  for (int e = threadIdx.x; e < 169; e += blockDim.x) P[(size_t)b * ld * ld + (size_t)(e / 13) * ld + (e % 13)] = Pxx[s * 169 + e];
  if (threadIdx.x < 13) x[(size_t)b * ld + threadIdx.x] = xv[s * 13 + threadIdx.x];
}

__global__ void k_get_vehicle(const double* __restrict__ x, const double* __restrict__ P, double* __restrict__ xv,
                              double* __restrict__ Pxx, int seq0, int ld) {
  const int s = blockIdx.x, b = seq0 + s;
  for (int e = threadIdx.x; e < 169; e += blockDim.x) Pxx[s * 169 + e] = P[(size_t)b * ld * ld + (size_t)(e / 13) * ld + (e % 13)];
  if (threadIdx.x < 13) xv[s * 13 + threadIdx.x] = x[(size_t)b * ld + threadIdx.x];
}

__global__ void k_ncc_score(const int* __restrict__ sums5, int count, double* __restrict__ score, double* __restrict__ sd0,
                            double* __restrict__ sd1) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  double a, b;
  score[i] = ncc_score(sums5[i * 5], sums5[i * 5 + 1], sums5[i * 5 + 2], sums5[i * 5 + 3], sums5[i * 5 + 4], &a, &b);
  sd0[i] = a; sd1[i] = b;
}

static int check_device() {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
    set_error("no HIP device visible: scenelib2_amd has no CPU fallback");
    return SL2_ERR_NO_DEVICE;
  }
  return SL2_OK;
}

template <typename T>
static int dmalloc(T** p, size_t count) {
  SL2_HIP(hipMalloc((void**)p, sizeof(T) * (count ? count : 1)));
  SL2_HIP(hipMemset(*p, 0, sizeof(T) * (count ? count : 1)));
  return SL2_OK;
}

template <typename T>
static int fetch_vec(std::vector<T>& v, const T* dev, size_t off, size_t n) {
  v.resize(n);
  SL2_HIP(hipMemcpy(v.data(), dev + off, sizeof(T) * n, hipMemcpyDeviceToHost));
  return SL2_OK;
}

// Engine-owned scratch of the accessors: a device buffer and a pinned host buffer that only ever grow.  (The accessors used
// to hipMalloc / hipFree per call - a device-wide synchronisation each - and leaked both buffers on an error return.)
static int acc_scratch(sl2_engine* e, size_t dev_bytes, size_t host_bytes) {
  sl2_engine* r = e->root;
  if (dev_bytes > r->acc_dev_bytes) {
    if (r->acc_dev) { SL2_HIP(hipFree(r->acc_dev)); r->acc_dev = nullptr; r->acc_dev_bytes = 0; }
    const size_t want = (dev_bytes + 4095) & ~(size_t)4095;
    SL2_HIP(hipMalloc(&r->acc_dev, want));
    r->acc_dev_bytes = want;
  }
  if (host_bytes > r->acc_host_bytes) {
    if (r->acc_host) { SL2_HIP(hipHostFree(r->acc_host)); r->acc_host = nullptr; r->acc_host_bytes = 0; }
    const size_t want = (host_bytes + 4095) & ~(size_t)4095;
    SL2_HIP(hipHostMalloc(&r->acc_host, want, hipHostMallocDefault));
    r->acc_host_bytes = want;
  }
  return SL2_OK;
}

}  // namespace sl2

#ifdef SL2_TESTING
#include "../../include/scenelib2_amd_testing.h"
#endif
using namespace sl2;

// Captured steps bake kernel choices, arguments and the groups' pointers in: every setter that changes one of them drops the
// graphs through here - after the device has finished with them (a replay may still be in flight on the engine's streams).
static int drop_step_graphs(sl2_engine* e) {
  if (e->step_graphs.empty()) return SL2_OK;
  SL2_HIP(hipSetDevice(e->device));
  { int rc = e->sync_all(); if (rc != SL2_OK) return rc; }
  for (auto& sg : e->step_graphs) hipGraphExecDestroy(sg.exec);
  e->step_graphs.clear();
  return SL2_OK;
}

// Release a group object and what it owns: its stream (unless it steps on the root's), its join event and its list of
// large search windows.  Also right for a half-built group.
static void free_group(sl2_engine* root, sl2_engine* g) {
  if (g->stream && g->stream != root->stream) hipStreamDestroy(g->stream);
  if (g->fork_event) hipEventDestroy(g->fork_event);
  if (g->srch_big) hipFree(g->srch_big);
  delete g;
}

// Build the group objects: shallow copies of the root whose per-sequence pointers start at
// `first` (seq_arrays_view) and whose B is the group's sequence count.  G == 1 -> a single group on the root stream.
static int build_groups(sl2_engine* e, int G) {
  for (sl2_engine* g : e->groups) free_group(e, g);
  e->groups.clear();
  if (G < 1) G = 1;
  if (G > e->B) G = e->B;
  const SeqDims dims = {(size_t)e->N, (size_t)e->ld, (size_t)e->mld, (size_t)e->nblk_max, (size_t)e->kpart, (size_t)e->pcap};
  for (int k = 0; k < G; ++k) {
    int first, count;
    group_range(e->B, G, k, &first, &count);
    sl2_engine* g = new sl2_engine();
    g->device = e->device; g->cam = e->cam; g->prm = e->prm;
    g->B = count; g->N = e->N; g->ld = e->ld; g->nsel_max = e->nsel_max; g->mld = e->mld; g->nblk_max = e->nblk_max;
    g->ppos = e->ppos; g->pcap = e->pcap; g->kpart = e->kpart;
    g->root = e; g->group_first = first;
    static_cast<SeqArrays&>(*g) = seq_arrays_view(*e, dims, first);
    const int rc = [&]() -> int {
      if (G == 1) g->stream = e->stream; else SL2_HIP(hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking));
      // the group's list of large search windows: count and counters start at zero and are returned to zero by k_search_score
      SL2_HIP(hipMalloc((void**)&g->srch_big, sizeof(int) * kSrchBigInts));
      SL2_HIP(hipMemsetAsync(g->srch_big, 0, sizeof(int) * kSrchBigParts, e->stream));      // (everything but the partial results)
      return SL2_OK;
    }();
    if (rc != SL2_OK) { free_group(e, g); return rc; }
    e->groups.push_back(g);
  }
  return SL2_OK;
}

// Order the group streams after everything already queued on the root stream (fork) ...
static int fork_groups(sl2_engine* e) {
  if (e->groups.size() == 1 && e->groups[0]->stream == e->stream) return SL2_OK;
  if (!e->fork_event) SL2_HIP(hipEventCreateWithFlags(&e->fork_event, hipEventDisableTiming));
  SL2_HIP(hipEventRecord(e->fork_event, e->stream));
  for (sl2_engine* g : e->groups) SL2_HIP(hipStreamWaitEvent(g->stream, e->fork_event, 0));
  return SL2_OK;
}
// ... and the root stream after the groups (join).
static int join_groups(sl2_engine* e) {
  if (e->groups.size() == 1 && e->groups[0]->stream == e->stream) return SL2_OK;
  // Always: the next thing queued on the root stream may be the host-frame copy into frames_buf (bind_frames), an
  // ingest copy into a device batch, or the caller's own work - all of which must come after the groups' kernels that
  // still read the previous frame.  (An engine-owned stream used to skip this: a plain C caller stepping with host
  // frames and groups > 1 then raced the copy against the previous step's search.)
  for (sl2_engine* g : e->groups) {
    if (!g->fork_event) SL2_HIP(hipEventCreateWithFlags(&g->fork_event, hipEventDisableTiming));
    SL2_HIP(hipEventRecord(g->fork_event, g->stream));
    SL2_HIP(hipStreamWaitEvent(e->stream, g->fork_event, 0));
  }
  return SL2_OK;
}

// Run `fn(group)` for every group between a fork and a join.
template <typename F>
static int for_each_group(sl2_engine* e, F fn) {
  int rc = fork_groups(e);
  if (rc != SL2_OK) return rc;
  for (sl2_engine* g : e->groups) {
    g->cur_frames = e->cur_frames ? e->cur_frames + (size_t)g->group_first * e->cur_stride : nullptr;
    g->cur_stride = e->cur_stride;
    if ((rc = fn(g)) != SL2_OK) return rc;
  }
  return join_groups(e);
}


int sl2_engine::timer_id(const char* name) {
  for (size_t i = 0; i < timers.size(); ++i)
    if (timers[i].name == name) return (int)i;
  KernelTimer t;
  t.name = name;
  timers.push_back(t);
  return (int)timers.size() - 1;
}

void sl2_engine::prof_begin(int id, hipStream_t st) {
  PendingEvent pe;
  pe.timer = id;
  for (int k = 0; k < 2; ++k) {
    hipEvent_t ev;
    if (!event_pool.empty()) { ev = event_pool.back(); event_pool.pop_back(); }
    else hipEventCreate(&ev);
    if (k == 0) pe.start = ev; else pe.stop = ev;
  }
  hipEventRecord(pe.start, st);
  pending.push_back(pe);
}

void sl2_engine::prof_end(hipStream_t st) { hipEventRecord(pending.back().stop, st); }

int sl2_engine::sync_all() {
  for (sl2_engine* g : root->groups) SL2_HIP(hipStreamSynchronize(g->stream));
  SL2_HIP(hipStreamSynchronize(root->stream));
  return SL2_OK;
}

int sl2_engine::fold_events() {
  if (pending.empty()) return SL2_OK;
  { int rc = sync_all(); if (rc != SL2_OK) return rc; }
  for (auto& pe : pending) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, pe.start, pe.stop) == hipSuccess) {
      timers[pe.timer].total_ms += ms;
      timers[pe.timer].launches += 1;
    }
    event_pool.push_back(pe.start);
    event_pool.push_back(pe.stop);
  }
  pending.clear();
  return SL2_OK;
}

extern "C" {

const char* sl2_last_error(void) { return g_err.c_str(); }

int sl2_api_version(void) { return SL2_API_VERSION; }

int sl2_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

// ---------------------------------------------------------------------------
// Where the large matrices land.  The same launch of k_build_AS takes 0.313-0.322 ms or 0.335-0.357 at configs[2], k_syrk
// 0.474 or 0.484, k_chol_left 0.168 or 0.172 - constant for the life of an allocation, different from one hipMalloc to the next
// even when the VIRTUAL addresses come out the same (two engines of one process, one after the other; rounds 4-5 saw it as "two
// modes from process to process").  What differs is the physical backing the driver happens to hand out; nothing in the API
// steers it.  So sl2_create asks: a probe - every sequence's workgroup streams its own part of a buffer, read and write, the way
// the update's kernels do - is timed on each of the four large matrices, up to kPlaceTries - 1 further sets are allocated BESIDE
// the first (held, not freed and re-allocated: a freed set tends to come back the same) and probed the same way, and the engine
// keeps the fastest buffer of each kind; the rest is freed.  For P more candidates are tried alone (up to 40 in all) until one
// stands out: about one in five is fast (probe 0.296-0.304 ms against 0.32-0.36), and it is P that k_build_AS streams.  k_syrk is
// then timed itself on the pairs of the best candidates of P and V^T (below).  Only where it can matter (kPlaceMinBytes of P), and
// never beyond a quarter of the free memory.  Same-box A/B: -2.1 / -2.2 % of the step (profiles/r06_placement_ab.txt).
// ---------------------------------------------------------------------------
constexpr int kPlaceTries = 10;
constexpr size_t kPlaceMinBytes = (size_t)256 << 20;
__global__ void __launch_bounds__(1024) k_place_probe(double* __restrict__ buf, size_t per_seq) {
  double* p = buf + (size_t)blockIdx.x * per_seq;
  for (size_t i = threadIdx.x; i < per_seq; i += blockDim.x) p[i] = p[i] + 0.0;      // (the buffers are all zeros at this point, and stay so)
}
static int probe_ms(sl2_engine* e, double* buf, size_t per_seq, float* ms_out) {
  hipEvent_t e0, e1;
  SL2_HIP(hipEventCreate(&e0));
  if (hipEventCreate(&e1) != hipSuccess) { hipEventDestroy(e0); set_error("hipEventCreate failed"); return SL2_ERR_HIP; }
  float best = 1e30f;
  hipError_t err = hipSuccess;
  for (int rep = 0; rep < 4 && err == hipSuccess; ++rep) {          // (the first one warms the translation caches)
    hipEventRecord(e0, e->stream);
    hipLaunchKernelGGL(k_place_probe, dim3(e->B), dim3(1024), 0, e->stream, buf, per_seq);
    hipEventRecord(e1, e->stream);
    err = hipEventSynchronize(e1);
    float ms = 0.0f;
    if (err == hipSuccess) err = hipEventElapsedTime(&ms, e0, e1);
    if (rep > 0 && ms < best) best = ms;
  }
  hipEventDestroy(e0); hipEventDestroy(e1);
  if (err != hipSuccess) { set_error(hipGetErrorString(err)); return SL2_ERR_HIP; }
  *ms_out = best;
  return SL2_OK;
}
static int place_large_matrices(sl2_engine* e) {
  const size_t B = e->B, ld = e->ld, mld = e->mld;
  if (sizeof(double) * B * ld * ld < kPlaceMinBytes) return SL2_OK;
  const size_t nP = ld * ld, nA = mld * ld, nS = mld * mld;            // doubles per sequence
  const size_t set_bytes = sizeof(double) * B * (nP + 2 * nA + nS);
  struct Cand { double* p; float ms; };
  std::vector<Cand> cP, cA, cS;                                         // (A^T and V^T are the same size: one pool)
  int rc = SL2_OK;
  auto add = [&](std::vector<Cand>& pool, double* p, size_t per_seq) {
    float ms = 0.0f;
    if (rc == SL2_OK) rc = probe_ms(e, p, per_seq, &ms);
    pool.push_back({p, ms});
  };
  add(cP, e->P, nP); add(cA, e->At, nA); add(cA, e->Vt, nA); add(cS, e->St, nS);
  // the candidates together never hold more than a quarter of what is free now
  size_t budget = 0;
  { size_t free_b = 0, total_b = 0; if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) budget = free_b / 4; }
  for (int t = 1; t < kPlaceTries && rc == SL2_OK; ++t) {
    if (set_bytes > budget) break;
    budget -= set_bytes;
    double *p = nullptr, *a = nullptr, *v = nullptr, *st = nullptr;
    if (dmalloc(&p, B * nP) != SL2_OK || dmalloc(&a, B * nA) != SL2_OK || dmalloc(&v, B * nA) != SL2_OK || dmalloc(&st, B * nS) != SL2_OK) {
      if (p) hipFree(p); if (a) hipFree(a); if (v) hipFree(v); if (st) hipFree(st);
      (void)hipGetLastError();                                          // (a set that does not fit: the engine keeps what it has)
      break;
    }
    add(cP, p, nP); add(cA, a, nA); add(cA, v, nA); add(cS, st, nS);
  }
  // The covariance is the one that decides k_build_AS's speed (and moves k_syrk's with it), and about one candidate in five is a
  // fast one: more of it alone, as many again.
  // (fast placements come in runs - twelve 800 MB slices of ONE allocation: ten slow, the last two fast, scripts/probes/place_probe.hip -
  // so the search goes on until a candidate stands out from the slowest by the 7 % that separates the two kinds, or 40 are held)
  auto p_found = [&]() {
    float lo = cP[0].ms, hi = cP[0].ms;
    for (const Cand& c : cP) { lo = c.ms < lo ? c.ms : lo; hi = c.ms > hi ? c.ms : hi; }
    return lo <= 0.93f * hi;
  };
  while ((int)cP.size() < 4 * kPlaceTries && !p_found() && rc == SL2_OK) {
    if (sizeof(double) * B * nP > budget) break;
    budget -= sizeof(double) * B * nP;
    double* p = nullptr;
    if (dmalloc(&p, B * nP) != SL2_OK) { (void)hipGetLastError(); break; }
    add(cP, p, nP);
  }
  auto by_ms = [](const Cand& x, const Cand& y) { return x.ms < y.ms; };
  std::stable_sort(cP.begin(), cP.end(), by_ms);
  std::stable_sort(cA.begin(), cA.end(), by_ms);
  std::stable_sort(cS.begin(), cS.end(), by_ms);
  // k_syrk, a third of the step, has a placement of its own that the streaming probe does not see (0.468-0.476 or 0.480-0.485 ms
  // with the same fast P): the kernel itself is the probe - on all-zero operands it does its full work and changes nothing - over
  // the pairs of the four best candidates of P and of V^T / A^T.
  size_t bp = 0, bv = 0;
  if (rc == SL2_OK && e->ld % 64 == 0) {
    std::vector<int> full_m(B, (int)(mld / 2)), full_n(B, e->N);
    hipMemcpy(e->m_count, full_m.data(), sizeof(int) * B, hipMemcpyHostToDevice);
    hipMemcpy(e->n_slots, full_n.data(), sizeof(int) * B, hipMemcpyHostToDevice);
    const size_t np4 = cP.size() < 4 ? cP.size() : 4, nv4 = cA.size() < 4 ? cA.size() : 4;
    float best = 1e30f, worst = 0.0f, best_score = 1e30f;
    hipEvent_t e0, e1;
    hipEventCreate(&e0); hipEventCreate(&e1);
    for (size_t i = 0; i < np4 && rc == SL2_OK; ++i)
      for (size_t j = 0; j < nv4 && rc == SL2_OK; ++j) {
        float t_best = 1e30f;
        for (int rep = 0; rep < 3 && rc == SL2_OK; ++rep) {
          hipEventRecord(e0, e->stream);
          rc = launch_syrk_on(e, cA[j].p, cP[i].p);
          hipEventRecord(e1, e->stream);
          if (hipEventSynchronize(e1) != hipSuccess) { set_error("placement probe failed"); rc = SL2_ERR_HIP; }
          float ms = 0.0f;
          hipEventElapsedTime(&ms, e0, e1);
          if (rep > 0 && ms < t_best) t_best = ms;
        }
        // (the pair is judged by k_syrk's time plus what its P costs k_build_AS, which streams it the way the first probe does)
        const float score = t_best + cP[i].ms;
        if (score < best_score) { best_score = score; best = t_best; bp = i; bv = j; }
        if (t_best > worst && t_best < 1e29f) worst = t_best;
      }
    hipEventDestroy(e0); hipEventDestroy(e1);
    hipMemset(e->m_count, 0, sizeof(int) * B);
    hipMemset(e->n_slots, 0, sizeof(int) * B);
    e->place_syrk_ms[0] = best; e->place_syrk_ms[1] = worst;
  }
  // A^T (written by k_build_AS, read once by the substitution): the best of what is left
  const size_t ba = (bv == 0) ? 1 : 0;
  e->P = cP[bp].p; e->Vt = cA[bv].p; e->At = cA[ba].p; e->St = cS[0].p;
  for (size_t i = 0; i < cP.size(); ++i) if (i != bp) hipFree(cP[i].p);
  for (size_t i = 0; i < cA.size(); ++i) if (i != bv && i != ba) hipFree(cA[i].p);
  for (size_t i = 1; i < cS.size(); ++i) hipFree(cS[i].p);
  e->place_worst_ms[0] = cP.back().ms; e->place_worst_ms[1] = cA.back().ms; e->place_worst_ms[2] = cS.back().ms;
  e->place_kept_ms[0] = cP[bp].ms; e->place_kept_ms[1] = cA[bv].ms; e->place_kept_ms[2] = cA[ba].ms; e->place_kept_ms[3] = cS[0].ms;
  e->place_candidates = (int)cP.size();
  return rc;
}

int sl2_create(const sl2_camera* cam, const sl2_params* params, int batch, int max_features, int device, void* stream,
               sl2_engine** out) {
  if (!cam || !params || !out || batch <= 0 || max_features <= 0) { set_error("sl2_create: bad argument"); return SL2_ERR_INVALID; }
  if (cam->width < 2 * SL2_PATCH_SIZE || cam->height < 2 * SL2_PATCH_SIZE) { set_error("sl2_create: image too small"); return SL2_ERR_INVALID; }
  int rc = check_device();
  if (rc != SL2_OK) return rc;
  SL2_HIP(hipSetDevice(device));
  sl2_engine* e = new sl2_engine();
  e->device = device;
  e->root = e;
  // everything below runs inside `build`: on any failure the partially built engine (stream, allocations) is released
  auto build = [&]() -> int {
  if (stream) { e->stream = (hipStream_t)stream; e->own_stream = false; }
  else { SL2_HIP(hipStreamCreate(&e->stream)); e->own_stream = true; }
  e->cam.width = cam->width; e->cam.height = cam->height; e->cam.fku = cam->fku; e->cam.fkv = cam->fkv;
  e->cam.u0 = cam->u0; e->cam.v0 = cam->v0; e->cam.kd1 = cam->kd1; e->cam.sd = cam->sd;
  e->prm = *params;
  if (e->prm.minimum_attempted_measurements_of_feature <= 0) e->prm.minimum_attempted_measurements_of_feature = 10;
  if (!(e->prm.successful_match_fraction > 0.0)) e->prm.successful_match_fraction = 0.5;
  e->B = batch; e->N = max_features;
  // partially initialised features in flight: params.max_features_to_init_at_once of them, the shipped value is 1
  e->kpart = params->max_features_to_init_at_once < 1 ? 1 : (params->max_features_to_init_at_once > kMaxPartial ? kMaxPartial : params->max_features_to_init_at_once);
  e->search_split = srch_split_default(e->cam.width, e->cam.height);
#ifdef SL2_TESTING   // TEST build: SL2_PANEL_FROM moves the block count from which the panel-wise / grouped forms take over
  if (const char* v = getenv("SL2_PANEL_FROM")) e->panel_from = e->group_from = atoi(v);
#endif
  // the state's columns and the innovation system's padded rows (sl2_update_plan.hpp)
  const UpdateSizes sizes = update_sizes(max_features, params->number_of_features_to_select, e->kpart, e->group_from, e->panel_from);
  e->ld = sizes.ld; e->ppos = sizes.ppos; e->nsel_max = sizes.nsel_max; e->mld = sizes.mld; e->nblk_max = sizes.nblk_max;
  {   // depth particles of the partially initialised feature: any count up to 1024 (the reference loops over any number)
    int np = params->number_of_particles;
    np = np < 1 ? 1 : (np > kMaxParticles ? kMaxParticles : np);
    e->pcap = round_up(np, 64);
  }
#ifndef SL2_TESTING
  if (!update_sizes_admitted(sizes)) {
    set_error("sl2_create: at most 676 feature slots (2048 state columns) and 512 features measured per frame");
    return SL2_ERR_CAPACITY;
  }
#endif
  const size_t B = batch;
  {   // every per-sequence array, zero-filled, in the order of the list (sl2_seq_arrays.hpp)
    const size_t N = max_features, ld = e->ld, mld = e->mld, nblk_max = e->nblk_max, kpart = e->kpart, pcap = e->pcap;
#define X(type, name, elems) { const int r = dmalloc(&e->name, B * (size_t)(elems)); if (r != SL2_OK) return r; }
    SL2_SEQ_ARRAYS(X)
#undef X
  }
  SL2_HIP(hipMemset(e->active, 1, B));                               // every sequence takes part until sl2_set_active_sequences says otherwise
  // (step_mark stays zero: nobody has stepped yet - sl2_get_step_stats)
  {   // every sequence starts on the engine's time step: nothing owed, no predict yet, catch-up off (sl2_set_delta_t)
    std::vector<double> rec(B * kSeqTimeDoubles, 0.0);
    for (size_t b = 0; b < B; ++b) rec[b * kSeqTimeDoubles + kSeqTimeNominal] = e->prm.delta_t;
    SL2_HIP(hipMemcpy(e->seq_time, rec.data(), sizeof(double) * rec.size(), hipMemcpyHostToDevice));
  }
  {   // every sequence starts with the engine's calibration (sl2_set_cameras)
    std::vector<double> rec(B * kSeqCamDoubles, 0.0);
    for (size_t b = 0; b < B; ++b) {
      double* c = &rec[b * kSeqCamDoubles];
      c[kSeqCamFku] = cam->fku; c[kSeqCamFkv] = cam->fkv; c[kSeqCamU0] = cam->u0; c[kSeqCamV0] = cam->v0;
      c[kSeqCamKd1] = cam->kd1; c[kSeqCamSd] = (double)cam->sd;
    }
    SL2_HIP(hipMemcpy(e->seq_cam, rec.data(), sizeof(double) * rec.size(), hipMemcpyHostToDevice));
    sl2_camera c0;
    memset(&c0, 0, sizeof(c0));      // (padding too: blobs and the checkpoint checks compare the struct's bytes)
    c0.width = cam->width; c0.height = cam->height; c0.fku = cam->fku; c0.fkv = cam->fkv; c0.u0 = cam->u0; c0.v0 = cam->v0;
    c0.kd1 = cam->kd1; c0.sd = cam->sd;
    e->cams_host.assign(B, c0);
  }
  SL2_HIP(hipMalloc((void**)&e->slots_max_dev, sizeof(int) * 2));
  SL2_HIP(hipMemset(e->slots_max_dev, 0, sizeof(int) * 2));
  SL2_HIP(hipHostMalloc((void**)&e->slots_mail, 2 * sizeof(unsigned long long), hipHostMallocMapped | hipHostMallocCoherent));
  e->slots_mail[0] = 0ull; e->slots_mail[1] = 0ull;
  SL2_HIP(hipHostGetDevicePointer((void**)&e->slots_mail_dev, e->slots_mail, 0));
  e->parts_mail = e->slots_mail + 1; e->parts_mail_dev = e->slots_mail_dev + 1;
  {  // srand48(0) in MonoSLAM::Init (monoslam.cpp:1968), one generator per sequence
    std::vector<unsigned long long> seeds(B, kRand48Seed0);
    SL2_HIP(hipMemcpy(e->rand48, seeds.data(), sizeof(unsigned long long) * B, hipMemcpyHostToDevice));
  }
  SL2_HIP(hipDeviceSynchronize());
  e->root = e;
#ifdef SL2_TESTING
  if (!getenv("SL2_NO_PLACE"))       // (TEST build: the same-box A/B of the placement, profiles/r06_placement_ab.txt)
#endif
  { int rc2 = place_large_matrices(e); if (rc2 != SL2_OK) return rc2; }
#ifdef SL2_TESTING
  if (getenv("SL2_DEBUG_PLACE")) fprintf(stderr, "PLACE %d candidates; kept P %.4f Vt %.4f At %.4f St %.4f; slowest P %.4f A %.4f St %.4f\n", e->place_candidates, e->place_kept_ms[0], e->place_kept_ms[1], e->place_kept_ms[2], e->place_kept_ms[3], e->place_worst_ms[0], e->place_worst_ms[1], e->place_worst_ms[2]);
#endif
  int G = 1;
#ifdef SL2_TESTING
  // Development switches of the TEST build of the library (libscenelib2_amd_test.so, scripts/variants.sh): the product
  // library never reads the environment - there the kernel variants are chosen through sl2_set_search_variant /
  // sl2_set_update_variant / sl2_set_groups only.
  if (const char* v = getenv("SL2_FWD_VARIANT")) e->fwd_variant = atoi(v);
  if (const char* v = getenv("SL2_CHOL_VARIANT")) e->chol_variant = atoi(v);
  if (const char* v = getenv("SL2_BUILD_VARIANT")) e->build_variant = atoi(v);
  if (const char* v = getenv("SL2_SEARCH_VARIANT")) e->search_variant = atoi(v);
  if (const char* v = getenv("SL2_BUILD_SPLIT")) e->build_split = atoi(v);
  if (const char* v = getenv("SL2_BUILD_AHEAD")) e->build_ahead = atoi(v);
  if (const char* v = getenv("SL2_SCORE_THREADS")) e->score_threads = atoi(v);
  if (getenv("SL2_NO_KSPLIT")) e->no_ksplit = 1;
  if (const char* v = getenv("SL2_SEARCH_CHUNK")) e->search_chunk = atoi(v);
  if (const char* v = getenv("SL2_SEARCH_LDS_PAD")) e->search_lds_pad = atoi(v);
  if (const char* v = getenv("SL2_BUILD_LDS_MIN")) e->build_lds_min = atoi(v);
  if (const char* v = getenv("SL2_CHOL_PANEL")) e->chol_panel = atoi(v);
  if (const char* v = getenv("SL2_FWD_GROUP")) e->fwd_group = atoi(v);
  if (const char* env = getenv("SL2_GROUPS")) if (atoi(env) > 0) G = atoi(env);
#endif
  {
    int rc2 = build_groups(e, G);
    if (rc2 != SL2_OK) return rc2;
  }
  return SL2_OK;
  };
  rc = build();
  if (rc != SL2_OK) { sl2_destroy(e); return rc; }
  *out = e;
  return SL2_OK;
}

int sl2_set_groups(sl2_engine* e, int groups) {
  if (!e || groups < 1) return SL2_ERR_INVALID;
  SL2_HIP(hipSetDevice(e->device));
  { int rc = e->sync_all(); if (rc != SL2_OK) return rc; }
  // captured steps carry the groups' pointers (srch_big is re-allocated per group below, the streams change): replaying one
  // after a rebuild would write through freed device memory
  { int rc = drop_step_graphs(e); if (rc != SL2_OK) return rc; }
  return build_groups(e, groups);
}

void sl2_destroy(sl2_engine* e) {
  if (!e) return;
  hipSetDevice(e->device);
  e->sync_all();
  for (sl2_engine* g : e->groups) free_group(e, g);
  if (e->fork_event) hipEventDestroy(e->fork_event);
  for (auto& sg : e->step_graphs) hipGraphExecDestroy(sg.exec);
#define X(type, name, elems) if (e->name) hipFree(e->name);
  SL2_SEQ_ARRAYS(X)
#undef X
  void* lazy[] = {e->frames_buf, e->score_map, e->me_big_list, e->init_uv};      // (allocated on first use)
  for (void* p : lazy) if (p) hipFree(p);
  release_checkpoint_staging(e);
  if (e->slots_max_dev) hipFree(e->slots_max_dev);
  if (e->stats_host) hipHostFree(e->stats_host);
  if (e->slots_mail) hipHostFree(e->slots_mail);
  if (e->snap_stage) hipFree(e->snap_stage);
  if (e->snap_host) hipHostFree(e->snap_host);
  if (e->snapb_stage) hipFree(e->snapb_stage);
  if (e->snapb_aux) hipFree(e->snapb_aux);
  if (e->snapb_aux_host) hipHostFree(e->snapb_aux_host);
  if (e->ovl_lists) hipFree(e->ovl_lists);
  if (e->ovl_images) hipFree(e->ovl_images);
  if (e->acc_dev) hipFree(e->acc_dev);
  if (e->acc_host) hipHostFree(e->acc_host);
  for (auto& pe : e->pending) { hipEventDestroy(pe.start); hipEventDestroy(pe.stop); }
  for (auto ev : e->event_pool) hipEventDestroy(ev);
  if (e->own_stream) hipStreamDestroy(e->stream);
  delete e;
}

int sl2_synchronize(sl2_engine* e) {
  if (!e) return SL2_ERR_INVALID;
  { int _rc = e->sync_all(); if (_rc != SL2_OK) return _rc; }
  return SL2_OK;
}
void* sl2_get_stream(sl2_engine* e) { return e ? (void*)e->stream : nullptr; }
int sl2_batch(const sl2_engine* e) { return e ? e->B : 0; }
int sl2_max_features(const sl2_engine* e) { return e ? e->N : 0; }

static int range_ok(sl2_engine* e, int seq0, int nseq) { return e && seq0 >= 0 && nseq > 0 && seq0 + nseq <= e->B; }

// The largest n_slots of the batch, read back: only where the caller has just synchronised anyway.
static int refresh_slots_exact(sl2_engine* e) {
  std::vector<int> slots(e->B);
  SL2_HIP(hipMemcpy(slots.data(), e->n_slots, sizeof(int) * e->B, hipMemcpyDeviceToHost));
  int mx = 0;
  for (int v : slots) mx = v > mx ? v : mx;
  e->slots_exact = mx;
  e->slots_exact_step = e->steps_done;
  return SL2_OK;
}

// Upper bound on n_slots of any sequence at the step about to be issued (step index steps_done), without touching the
// device.  n_slots grows only in the feature-initialisation tail of a step (at most kpart per step and sequence, and only once
// feature initialisation is in use), in sl2_add_known_features and in the two "initialise feature" calls - the last two
// synchronise and read the exact value.  In between, finalize's mailbox (max over the batch as of step t - 1, published during
// step t) follows the device with a lag of however many steps the caller keeps in flight.
static int slots_upper_bound(const sl2_engine* e) {
  const long long s = e->steps_done;
  const long long grow = e->mapping_used ? e->kpart : 0;
  long long best = (long long)e->slots_exact + grow * (s - e->slots_exact_step);
  const unsigned long long mail = __atomic_load_n(e->slots_mail, __ATOMIC_ACQUIRE);
  const long long t = (long long)(mail >> 32);        // published while finalizing step t: the maximum of step t - 1
  if (t >= 1 && t - 1 >= e->slots_exact_step && t - 1 < s) {
    const long long viaMail = (long long)(mail & 0xffffffffull) + grow * (s - (t - 1));
    if (viaMail < best) best = viaMail;
  }
  return best > 1000000 ? 1000000 : (int)best;
}

// What the host knows about the partially initialised features the step about to be issued (index steps_done) starts with:
// 1 = none, 2 = every partial slot taken, 0 = not known (launch_mapping then issues every launch).  Known means: the step before
// it ran the feature-initialisation tail, whose k_map_update reported the count it left (one-sequence engines only: the report
// is a plain store of the one workgroup), the report has arrived, and no feature was initialised or deleted by hand since.  A
// caller who queues steps ahead of the device sees a report that is not current and gets the full set of launches - never a
// wrong skip.
static int parts_state_for_step(const sl2_engine* e) {
  if (e->B != 1 || !e->mapping_used || e->step_fusion == 0 || e->parts_block_step == e->steps_done || e->steps_done <= 0) return 0;
  const unsigned long long mail = __atomic_load_n(e->parts_mail, __ATOMIC_ACQUIRE);
  if ((long long)(mail >> 32) != e->steps_done) return 0;
  const long long left = (long long)(mail & 0xffffffffull);
  return left == 0 ? 1 : (left >= e->kpart ? 2 : 0);
}

int sl2_set_vehicle_state(sl2_engine* e, int seq0, int nseq, const double* xv, const double* Pxx) {
  if (!range_ok(e, seq0, nseq) || !xv || !Pxx) return SL2_ERR_INVALID;
  SL2_HIP(hipSetDevice(e->device));
  { int _rc = e->sync_all(); if (_rc != SL2_OK) return _rc; }
  const size_t nx = (size_t)13 * nseq, nP = (size_t)169 * nseq;
  { int _rc = acc_scratch(e, sizeof(double) * (nx + nP), 0); if (_rc != SL2_OK) return _rc; }
  double* dxv = (double*)e->acc_dev;
  double* dP = dxv + nx;
  SL2_HIP(hipMemcpyAsync(dxv, xv, sizeof(double) * nx, hipMemcpyHostToDevice, e->stream));
  SL2_HIP(hipMemcpyAsync(dP, Pxx, sizeof(double) * nP, hipMemcpyHostToDevice, e->stream));
  hipLaunchKernelGGL(k_set_vehicle, dim3(nseq), dim3(64), 0, e->stream, e->x, e->P, dxv, dP, seq0, e->ld);
  SL2_HIP(hipGetLastError());
  { int _rc = e->sync_all(); if (_rc != SL2_OK) return _rc; }
  return SL2_OK;
}

int sl2_get_vehicle_state(sl2_engine* e, int seq0, int nseq, double* xv, double* Pxx) {
  if (!range_ok(e, seq0, nseq) || !xv || !Pxx) return SL2_ERR_INVALID;
  SL2_HIP(hipSetDevice(e->device));
  const size_t nx = (size_t)13 * nseq, nP = (size_t)169 * nseq;
  { int _rc = acc_scratch(e, sizeof(double) * (nx + nP), sizeof(double) * (nx + nP)); if (_rc != SL2_OK) return _rc; }
  double* dxv = (double*)e->acc_dev;
  double* dP = dxv + nx;
  // one gather kernel, ONE copy into the engine's pinned scratch, one synchronisation (the root stream is ordered behind
  // the sequence groups' streams by the join at the end of every stepping call)
  hipLaunchKernelGGL(k_get_vehicle, dim3(nseq), dim3(64), 0, e->stream, e->x, e->P, dxv, dP, seq0, e->ld);
  SL2_HIP(hipGetLastError());
  SL2_HIP(hipMemcpyAsync(e->acc_host, dxv, sizeof(double) * (nx + nP), hipMemcpyDeviceToHost, e->stream));
  { int _rc = e->sync_all(); if (_rc != SL2_OK) return _rc; }
  memcpy(xv, e->acc_host, sizeof(double) * nx);
  memcpy(Pxx, (const double*)e->acc_host + nx, sizeof(double) * nP);
  return SL2_OK;
}

int sl2_set_feature_covariances(sl2_engine* e, int seq0, int nseq, int nfeat, const double* Pyy) {
  if (!range_ok(e, seq0, nseq) || nfeat <= 0 || nfeat > e->N || !Pyy) return SL2_ERR_INVALID;
  SL2_HIP(hipSetDevice(e->device));
  { int _rc = e->sync_all(); if (_rc != SL2_OK) return _rc; }
  const size_t cnt = (size_t)nseq * nfeat * 9;
  { int _rc = acc_scratch(e, sizeof(double) * cnt, 0); if (_rc != SL2_OK) return _rc; }
  double* d = (double*)e->acc_dev;
  SL2_HIP(hipMemcpyAsync(d, Pyy, sizeof(double) * cnt, hipMemcpyHostToDevice, e->stream));
  hipLaunchKernelGGL(k_set_feature_cov, dim3(nseq), dim3(256), 0, e->stream, e->P, d, seq0, nfeat, e->ld);
  SL2_HIP(hipGetLastError());
  { int _rc = e->sync_all(); if (_rc != SL2_OK) return _rc; }
  return SL2_OK;
}

int sl2_add_known_features(sl2_engine* e, int seq0, int nseq, int nfeat, const double* y, const double* xp_org,
                           const uint8_t* patches) {
  if (!range_ok(e, seq0, nseq) || nfeat <= 0 || !y || !xp_org || !patches) return SL2_ERR_INVALID;
  SL2_HIP(hipSetDevice(e->device));
  { int _rc = e->sync_all(); if (_rc != SL2_OK) return _rc; }
  std::vector<int> slots(nseq);
  SL2_HIP(hipMemcpy(slots.data(), e->n_slots + seq0, sizeof(int) * nseq, hipMemcpyDeviceToHost));
  bool lacking = false;
  for (int s = 0; s < nseq; ++s) lacking = lacking || slots[s] + nfeat > e->N;
  if (lacking) {        // slots of deleted features are given back first (the reference's feature_list_ simply shrinks)
    int rc = for_each_group(e, [nfeat](sl2_engine* g) { return launch_compact_slots(g, nfeat); });     // every sequence group
    if (rc != SL2_OK) return rc;
    { int _rc = e->sync_all(); if (_rc != SL2_OK) return _rc; }
    SL2_HIP(hipMemcpy(slots.data(), e->n_slots + seq0, sizeof(int) * nseq, hipMemcpyDeviceToHost));
  }
  for (int s = 0; s < nseq; ++s)
    if (slots[s] + nfeat > e->N) { set_error("sl2_add_known_features: feature capacity exceeded"); return SL2_ERR_CAPACITY; }
  const size_t cnt = (size_t)nseq * nfeat;
  { int _rc = acc_scratch(e, sizeof(double) * 10 * cnt + 121 * cnt, 0); if (_rc != SL2_OK) return _rc; }
  double* dy = (double*)e->acc_dev;
  double* dxp = dy + 3 * cnt;
  uint8_t* dp = (uint8_t*)(dxp + 7 * cnt);
  SL2_HIP(hipMemcpyAsync(dy, y, sizeof(double) * 3 * cnt, hipMemcpyHostToDevice, e->stream));
  SL2_HIP(hipMemcpyAsync(dxp, xp_org, sizeof(double) * 7 * cnt, hipMemcpyHostToDevice, e->stream));
  SL2_HIP(hipMemcpyAsync(dp, patches, 121 * cnt, hipMemcpyHostToDevice, e->stream));
  hipLaunchKernelGGL(k_add_features, dim3(nseq), dim3(64), 0, e->stream, e->x, e->xp_org, e->patch, e->patch_sums, e->f_flags,
                     e->n_slots, e->attempted, e->successful, e->f_label, e->next_label, dy, dxp, dp, seq0, nfeat, e->N, e->ld);
  SL2_HIP(hipGetLastError());
  { int _rc = e->sync_all(); if (_rc != SL2_OK) return _rc; }
  return refresh_slots_exact(e);
}

// ------------------------------------------------------------------- stepping a subset of the batch

// The host form travels in the launch's own arguments (kActiveChunk sequences a launch, a bit each): the caller's array is read
// before the call returns whatever kind of memory it is, nothing is staged in a buffer a later call could overwrite while steps
// are still queued ahead of this one, and nothing waits for the device.
constexpr int kActiveChunk = 2048;
struct ActiveBits { unsigned w[kActiveChunk / 32]; };
__global__ void __launch_bounds__(256) k_set_active_bits(uint8_t* __restrict__ active, ActiveBits bits, int count) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < count) active[i] = (uint8_t)((bits.w[i >> 5] >> (i & 31)) & 1u);
}
__global__ void __launch_bounds__(256) k_set_active_dev(uint8_t* __restrict__ active, const uint8_t* __restrict__ src, int count) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < count) active[i] = src[i] ? 1 : 0;
}

int sl2_set_active_sequences(sl2_engine* e, int seq0, int nseq, const uint8_t* active, int on_device) {
  if (!range_ok(e, seq0, nseq) || !active) return SL2_ERR_INVALID;
  SL2_HIP(hipSetDevice(e->device));
  // on the engine's stream: behind the steps already queued (every stepping call joins the groups' streams back into it), in
  // front of the next one (which forks from it); outside any captured step - the mask is data a replayed graph reads
  if (on_device) {
    hipLaunchKernelGGL(k_set_active_dev, dim3((nseq + 255) / 256), dim3(256), 0, e->stream, e->active + seq0, active, nseq);
    SL2_HIP(hipGetLastError());
    return SL2_OK;
  }
  for (int c0 = 0; c0 < nseq; c0 += kActiveChunk) {
    const int cnt = nseq - c0 < kActiveChunk ? nseq - c0 : kActiveChunk;
    ActiveBits bits;
    memset(&bits, 0, sizeof(bits));
    for (int i = 0; i < cnt; ++i) if (active[c0 + i]) bits.w[i >> 5] |= 1u << (i & 31);
    hipLaunchKernelGGL(k_set_active_bits, dim3((cnt + 255) / 256), dim3(256), 0, e->stream, e->active + seq0 + c0, bits, cnt);
    SL2_HIP(hipGetLastError());
  }
  return SL2_OK;
}

int sl2_get_active_sequences(sl2_engine* e, int seq0, int nseq, uint8_t* active) {
  if (!range_ok(e, seq0, nseq) || !active) return SL2_ERR_INVALID;
  SL2_HIP(hipSetDevice(e->device));
  { int _rc = e->sync_all(); if (_rc != SL2_OK) return _rc; }
  SL2_HIP(hipMemcpy(active, e->active + seq0, (size_t)nseq, hipMemcpyDeviceToHost));
  return SL2_OK;
}

// ------------------------------------------------------------------- the per-sequence time step

// Like the mask, the host form travels in the launch's own arguments (kDtChunk sequences a launch): consumed before the call
// returns, nothing staged, nothing waited for.  A valid step is finite and > 0; the host form has refused anything else
// before it launches, the device form leaves such a sequence as it was.
constexpr int kDtChunk = 256;
struct DtChunk { double v[kDtChunk]; };
__device__ __forceinline__ void set_dt_one(double* __restrict__ rec, double v) {
  if (!(v > 0.0) || !(v <= 1.7976931348623157e308)) return;       // NaN, <= 0, infinite
  rec[kSeqTimeNominal] = v;
  rec[kSeqTimeOwed] = 0.0;
}
__global__ void __launch_bounds__(256) k_set_dt_args(double* __restrict__ seq_time, DtChunk c, int count) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < count) set_dt_one(seq_time + (size_t)i * kSeqTimeDoubles, c.v[i]);
}
__global__ void __launch_bounds__(256) k_set_dt_dev(double* __restrict__ seq_time, const double* __restrict__ src, int count) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < count) set_dt_one(seq_time + (size_t)i * kSeqTimeDoubles, src[i]);
}
__global__ void __launch_bounds__(256) k_set_catch_up(double* __restrict__ seq_time, int enabled, int count) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  double* rec = seq_time + (size_t)i * kSeqTimeDoubles;
  rec[kSeqTimeCatchUp] = enabled ? 1.0 : 0.0;
  if (!enabled) rec[kSeqTimeOwed] = 0.0;
}

int sl2_set_delta_t(sl2_engine* e, int seq0, int nseq, const double* dt, int on_device) {
  if (!range_ok(e, seq0, nseq) || !dt) return SL2_ERR_INVALID;
  SL2_HIP(hipSetDevice(e->device));
  // on the engine's stream, outside any captured step, like the mask (sl2_set_active_sequences): the record is data a replayed
  // graph reads
  double* rec0 = e->seq_time + (size_t)seq0 * kSeqTimeDoubles;
  if (on_device) {
    hipLaunchKernelGGL(k_set_dt_dev, dim3((nseq + 255) / 256), dim3(256), 0, e->stream, rec0, dt, nseq);
    SL2_HIP(hipGetLastError());
    return SL2_OK;
  }
  for (int i = 0; i < nseq; ++i)
    if (!std::isfinite(dt[i]) || !(dt[i] > 0.0)) { set_error("sl2_set_delta_t: a time step must be finite and > 0"); return SL2_ERR_INVALID; }
  for (int c0 = 0; c0 < nseq; c0 += kDtChunk) {
    const int cnt = nseq - c0 < kDtChunk ? nseq - c0 : kDtChunk;
    DtChunk c;
    memset(&c, 0, sizeof(c));
    memcpy(c.v, dt + c0, sizeof(double) * cnt);
    hipLaunchKernelGGL(k_set_dt_args, dim3((cnt + 255) / 256), dim3(256), 0, e->stream, rec0 + (size_t)c0 * kSeqTimeDoubles, c, cnt);
    SL2_HIP(hipGetLastError());
  }
  return SL2_OK;
}

int sl2_get_delta_t(sl2_engine* e, int seq0, int nseq, double* dt, double* owed, double* last_used) {
  if (!range_ok(e, seq0, nseq) || !dt) return SL2_ERR_INVALID;
  SL2_HIP(hipSetDevice(e->device));
  { int _rc = e->sync_all(); if (_rc != SL2_OK) return _rc; }
  std::vector<double> rec;
  { int _rc = fetch_vec(rec, e->seq_time, (size_t)seq0 * kSeqTimeDoubles, (size_t)nseq * kSeqTimeDoubles); if (_rc != SL2_OK) return _rc; }
  for (int i = 0; i < nseq; ++i) {
    dt[i] = rec[(size_t)i * kSeqTimeDoubles + kSeqTimeNominal];
    if (owed) owed[i] = rec[(size_t)i * kSeqTimeDoubles + kSeqTimeOwed];
    if (last_used) last_used[i] = rec[(size_t)i * kSeqTimeDoubles + kSeqTimeUsed];
  }
  return SL2_OK;
}

int sl2_set_pause_catch_up(sl2_engine* e, int enabled) {
  if (!e) return SL2_ERR_INVALID;
  SL2_HIP(hipSetDevice(e->device));
  hipLaunchKernelGGL(k_set_catch_up, dim3((e->B + 255) / 256), dim3(256), 0, e->stream, e->seq_time, enabled ? 1 : 0, e->B);
  SL2_HIP(hipGetLastError());
  return SL2_OK;
}

// ------------------------------------------------------------------- the per-sequence camera calibration

// The six intrinsics of kCamChunk sequences travel in one launch's own arguments, like the time steps above: 64 x 48 bytes
// = 3 KB, under the 4 KB a launch may carry.  Everything was validated on the host before the first launch.
constexpr int kCamChunk = 64;
struct CamChunk { double v[kCamChunk][6]; };
static_assert(sizeof(CamChunk) + 64 <= 4096, "a chunk and the two other arguments must fit the kernel-argument segment");
__global__ void __launch_bounds__(64) k_set_cam_args(double* __restrict__ seq_cam, CamChunk c, int count) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  double* rec = seq_cam + (size_t)i * kSeqCamDoubles;
  for (int k = 0; k < 6; ++k) rec[k] = c.v[i][k];       // (kSeqCamFku .. kSeqCamSd are places 0 .. 5; the two spare words stay 0)
}

int sl2_set_cameras(sl2_engine* e, int seq0, int nseq, const sl2_camera* cams) {
  if (!range_ok(e, seq0, nseq) || !cams) return SL2_ERR_INVALID;
  for (int i = 0; i < nseq; ++i) {
    const sl2_camera& c = cams[i];
    if (c.width != e->cam.width || c.height != e->cam.height) {
      set_error("sl2_set_cameras: the image size is the engine's; a sequence's camera cannot change it"); return SL2_ERR_INVALID;
    }
    if (!std::isfinite(c.fku) || !std::isfinite(c.fkv) || !std::isfinite(c.u0) || !std::isfinite(c.v0) || !std::isfinite(c.kd1) ||
        c.fku == 0.0 || c.fkv == 0.0 || c.sd < 0) {
      set_error("sl2_set_cameras: fku, fkv, u0, v0 and kd1 must be finite, fku and fkv not 0, sd >= 0"); return SL2_ERR_INVALID;
    }
  }
  SL2_HIP(hipSetDevice(e->device));
  // on the engine's stream, outside any captured step, like the mask and the time step: the record is data a replayed graph reads
  for (int c0 = 0; c0 < nseq; c0 += kCamChunk) {
    const int cnt = nseq - c0 < kCamChunk ? nseq - c0 : kCamChunk;
    CamChunk ch;
    memset(&ch, 0, sizeof(ch));
    for (int i = 0; i < cnt; ++i) {
      const sl2_camera& c = cams[c0 + i];
      double* v = ch.v[i];
      v[kSeqCamFku] = c.fku; v[kSeqCamFkv] = c.fkv; v[kSeqCamU0] = c.u0; v[kSeqCamV0] = c.v0; v[kSeqCamKd1] = c.kd1; v[kSeqCamSd] = (double)c.sd;
    }
    hipLaunchKernelGGL(k_set_cam_args, dim3(1), dim3(64), 0, e->stream, e->seq_cam + (size_t)(seq0 + c0) * kSeqCamDoubles, ch, cnt);
    SL2_HIP(hipGetLastError());
    for (int i = 0; i < cnt; ++i) {      // the mirror follows launch by launch: it never says more than was queued
      sl2_camera& m = e->cams_host[seq0 + c0 + i];
      const sl2_camera& c = cams[c0 + i];
      m.fku = c.fku; m.fkv = c.fkv; m.u0 = c.u0; m.v0 = c.v0; m.kd1 = c.kd1; m.sd = c.sd;
    }
  }
  return SL2_OK;
}

int sl2_get_cameras(sl2_engine* e, int seq0, int nseq, sl2_camera* cams) {
  if (!range_ok(e, seq0, nseq) || !cams) return SL2_ERR_INVALID;
  for (int i = 0; i < nseq; ++i) cams[i] = e->cams_host[seq0 + i];      // (the host's mirror: no wait for the device)
  return SL2_OK;
}

// ------------------------------------------------------------------- stepping

static int bind_frames(sl2_engine* e, const uint8_t* frames, size_t seq_stride, int on_device) {
  const size_t fb = (size_t)e->cam.width * e->cam.height;
  if (!frames || seq_stride < fb) { set_error("frames: null pointer or seq_stride < width*height"); return SL2_ERR_INVALID; }
  if (on_device) {
    e->cur_frames = frames;
    e->cur_stride = seq_stride;
    return SL2_OK;
  }
  if (!e->frames_buf) SL2_HIP(hipMalloc((void**)&e->frames_buf, fb * e->B));
  SL2_HIP(hipMemcpy2DAsync(e->frames_buf, fb, frames, seq_stride, fb, e->B, hipMemcpyHostToDevice, e->stream));
  e->cur_frames = e->frames_buf;
  e->cur_stride = fb;
  return SL2_OK;
}

int sl2_set_search_variant(sl2_engine* e, int variant) {
  if (!e || variant < 0 || variant > 1) return SL2_ERR_INVALID;
  { int rc = drop_step_graphs(e); if (rc != SL2_OK) return rc; }
  e->search_variant = variant;
  return SL2_OK;
}

int sl2_set_search_split(sl2_engine* e, int min_bands) {
  if (!e || min_bands < 0) return SL2_ERR_INVALID;
  { int rc = drop_step_graphs(e); if (rc != SL2_OK) return rc; }        // the threshold is a kernel argument of the captured k_select
  e->search_split = min_bands;
  return SL2_OK;
}

int sl2_set_step_fusion(sl2_engine* e, int enabled) {
  if (!e) return SL2_ERR_INVALID;
  { int rc = drop_step_graphs(e); if (rc != SL2_OK) return rc; }
  e->step_fusion = enabled == 2 ? 2 : (enabled ? 1 : 0);
  return SL2_OK;
}

#ifdef SL2_CHOL_TRACE
// development only: cycle stamps [B][4 waves][8 J][4 slots] + HW_ID [B][4]
int sl2_debug_chol_trace(sl2_engine* e, long long* out, size_t n) {
  const size_t total = (size_t)e->B * 4 * 8 * 4 + (size_t)e->B * 4;
  if (!e->chol_trace) {
    SL2_HIP(hipMalloc(&e->chol_trace, total * 8));
    SL2_HIP(hipMemset(e->chol_trace, 0, total * 8));
    return SL2_OK;
  }
  SL2_HIP(hipDeviceSynchronize());
  SL2_HIP(hipMemcpy(out, e->chol_trace, (n < total ? n : total) * 8, hipMemcpyDeviceToHost));
  return SL2_OK;
}
#endif

int sl2_set_update_variant(sl2_engine* e, int chol_variant, int fwd_variant) {
  if (!e || chol_variant < 0 || chol_variant > 1 || fwd_variant < 0 || fwd_variant > 1) return SL2_ERR_INVALID;
#ifndef SL2_TESTING
  if (chol_variant != 1 || fwd_variant != 1) {
    set_error("sl2_set_update_variant: the superseded kernel variants are compiled into the TEST build of the library only "
              "(libscenelib2_amd_test.so); this library runs chol_variant = 1, fwd_variant = 1");
    return SL2_ERR_INVALID;
  }
#endif
  { int rc = drop_step_graphs(e); if (rc != SL2_OK) return rc; }
  e->chol_variant = chol_variant;
  e->fwd_variant = fwd_variant;
  return SL2_OK;
}

int sl2_kalman_filter_predict(sl2_engine* e) {
  if (!e) return SL2_ERR_INVALID;
  SL2_HIP(hipSetDevice(e->device));
  return for_each_group(e, [](sl2_engine* g) { return launch_predict(g); });
}

int sl2_auto_select_n_features(sl2_engine* e, int n) {
  if (!e) return SL2_ERR_INVALID;
  SL2_HIP(hipSetDevice(e->device));
  return for_each_group(e, [n](sl2_engine* g) {
    int rc = launch_feature_prediction(g);
    if (rc != SL2_OK) return rc;
    return launch_select(g, n);
  });
}

int sl2_make_measurements(sl2_engine* e, const uint8_t* frames, size_t seq_stride, int frames_on_device) {
  if (!e) return SL2_ERR_INVALID;
  SL2_HIP(hipSetDevice(e->device));
  int rc = bind_frames(e, frames, seq_stride, frames_on_device);
  if (rc != SL2_OK) return rc;
  return for_each_group(e, [](sl2_engine* g) { return launch_search(g); });
}

int sl2_kalman_filter_update(sl2_engine* e) {
  if (!e) return SL2_ERR_INVALID;
  SL2_HIP(hipSetDevice(e->device));
  return for_each_group(e, [](sl2_engine* g) { return launch_update(g); });
}

int sl2_finish_step(sl2_engine* e, int save_trajectory) {
  if (!e) return SL2_ERR_INVALID;
  SL2_HIP(hipSetDevice(e->device));
  int rc = for_each_group(e, [=](sl2_engine* g) { return launch_finalize(g, save_trajectory); });
  if (rc == SL2_OK) e->steps_done += 1;
  return rc;
}


// Feature initialisation is in use from now on (enable_mapping, or one of the two "initialise feature" entry points): checks
// what this engine supports and allocates the per-pixel maps of the multi-ellipse search.
static int enable_feature_initialisation(sl2_engine* e) {
  if (e->mapping_used) return SL2_OK;
  // data/SceneLib2.cfg:62 ships max_features_to_init_at_once = 1; up to kMaxPartial partially initialised features per sequence
  // are carried (six state columns each, reserved at sl2_create)
  if (e->prm.max_features_to_init_at_once < 1 || e->prm.max_features_to_init_at_once > kMaxPartial ||
      e->prm.number_of_particles < 1 || e->prm.number_of_particles > kMaxParticles) {
    set_error("feature initialisation: needs 1 <= max_features_to_init_at_once <= 4 and 1 <= number_of_particles <= 1024");
    return SL2_ERR_INVALID;
  }
  if (e->groups.size() > 1) { set_error("feature initialisation: not available with sequence groups (sl2_set_groups > 1)"); return SL2_ERR_INVALID; }
  {   // k_map_update keeps the particle list in dynamic LDS (96 B per particle) next to ~1 KB of static LDS: say so here
      // rather than fail at the first launch (gfx950 has 160 KB per workgroup; the check is for whatever device this is)
    hipDeviceProp_t prop;
    SL2_HIP(hipGetDeviceProperties(&prop, e->device));
    const size_t need = sizeof(double) * kParticleDoubles * (size_t)e->prm.number_of_particles + 2048;
    if (need > prop.sharedMemPerBlock) {
      char buf[200];
      snprintf(buf, sizeof(buf), "feature initialisation: number_of_particles = %d needs %zu bytes of LDS per workgroup, the device has %zu",
               e->prm.number_of_particles, need, (size_t)prop.sharedMemPerBlock);
      set_error(buf);
      return SL2_ERR_CAPACITY;
    }
  }
  if (!e->score_map) {
    const size_t px = (size_t)e->B * e->kpart * e->cam.width * e->cam.height;
    SL2_HIP(hipMalloc((void**)&e->score_map, sizeof(double) * px));
    SL2_HIP(hipMalloc((void**)&e->me_big_list, sizeof(int) * ((size_t)e->B * e->kpart + 1)));
    e->me_big_count = e->me_big_list + (size_t)e->B * e->kpart;
    SL2_HIP(hipMemsetAsync(e->me_big_list, 0, sizeof(int) * ((size_t)e->B * e->kpart + 1), e->stream));
  }
  e->mapping_used = true;
  return SL2_OK;
}

// Feature initialisation runs on group 0, the whole batch (enable_feature_initialisation refuses sequence groups): hand it the
// frame binding (the buffers allocated on first use are read through root).
static sl2_engine* mapping_group(sl2_engine* e) {
  sl2_engine* g = e->groups[0];
  g->cur_frames = e->cur_frames; g->cur_stride = e->cur_stride;
  return g;
}

static int initialise_common(sl2_engine* e, const uint8_t* frames, size_t seq_stride, int frames_on_device, const int32_t* uv,
                             int32_t* created) {
  if (!e) return SL2_ERR_INVALID;
  SL2_HIP(hipSetDevice(e->device));
  int rc;
  if ((rc = enable_feature_initialisation(e)) != SL2_OK) return rc;
  if ((rc = bind_frames(e, frames, seq_stride, frames_on_device)) != SL2_OK) return rc;
  sl2_engine* g = mapping_group(e);
  if (uv) {
    if (!e->init_uv) SL2_HIP(hipMalloc((void**)&e->init_uv, sizeof(int) * 2 * e->B));
    // the caller's buffer may be pinned or registered memory, for which an asynchronous copy really is asynchronous: the copy
    // is waited for, so that uv need not outlive the call (a few hundred bytes; the call synchronises for `created` anyway)
    SL2_HIP(hipMemcpyAsync(e->init_uv, uv, sizeof(int) * 2 * e->B, hipMemcpyHostToDevice, e->stream));
    SL2_HIP(hipStreamSynchronize(e->stream));
    rc = launch_manual_init(g, e->init_uv);
  } else {
    rc = launch_auto_init(g);
  }
  if (rc != SL2_OK) return rc;
  e->parts_block_step = e->steps_done;       // the next step starts with a partial feature k_map_update has not reported
  { int rc2 = drop_step_graphs(e); if (rc2 != SL2_OK) return rc2; }     // captured steps were recorded without the feature-initialisation tail
  // (a button press: the call synchronises, and takes the exact map sizes while it is at it)
  { int _rc = e->sync_all(); if (_rc != SL2_OK) return _rc; }
  { int _rc = refresh_slots_exact(e); if (_rc != SL2_OK) return _rc; }
  if (created) {
    std::vector<int> pi((size_t)e->B * kPartInts);
    SL2_HIP(hipMemcpy(pi.data(), e->part_i, sizeof(int) * pi.size(), hipMemcpyDeviceToHost));
    for (int b = 0; b < e->B; ++b) created[b] = pi[(size_t)b * kPartInts + kPartCreated];
  }
  return SL2_OK;
}

int sl2_initialise_feature(sl2_engine* e, const uint8_t* frames, size_t seq_stride, int frames_on_device, const int32_t* uv,
                           int32_t* created) {
  if (!uv) return SL2_ERR_INVALID;
  return initialise_common(e, frames, seq_stride, frames_on_device, uv, created);
}

int sl2_initialise_auto_feature(sl2_engine* e, const uint8_t* frames, size_t seq_stride, int frames_on_device, int32_t* created) {
  return initialise_common(e, frames, seq_stride, frames_on_device, nullptr, created);
}

int sl2_go_one_step(sl2_engine* e, const uint8_t* frames, size_t seq_stride, int frames_on_device, int save_trajectory,
                    int enable_mapping) {
  if (!e) return SL2_ERR_INVALID;
  SL2_HIP(hipSetDevice(e->device));
  int rc;
  if (enable_mapping && !e->mapping_used && (rc = enable_feature_initialisation(e)) != SL2_OK) return rc;
  if ((rc = bind_frames(e, frames, seq_stride, frames_on_device)) != SL2_OK) return rc;
  const int nsel = e->prm.number_of_features_to_select;
  // What this step launches, decided once (sl2_step_plan.hpp): the launch list walks the plan, and a captured step is keyed by it.
  const StepShape shape = {e->N, e->ld, e->mld, e->kpart, e->step_fusion, e->mapping_used, {e->groups.front()->B, e->groups.back()->B}};
  const StepPlan plan = make_step_plan(shape, slots_upper_bound(e), e->mapping_used ? parts_state_for_step(e) : 0, save_trajectory, enable_mapping);
  auto issue = [=]() -> int {
    int r = for_each_group(e, [=](sl2_engine* g) {
      const GroupPlan& gp = plan.group[g->B == shape.group_B[0] ? 0 : 1];
      int q;
      if (gp.small_front) {
        if ((q = launch_small_front(g, nsel)) != SL2_OK) return q;
      } else {
        if ((q = launch_predict(g)) != SL2_OK) return q;
        if ((q = launch_feature_prediction(g)) != SL2_OK) return q;
        if ((q = launch_select(g, nsel)) != SL2_OK) return q;
      }
      if (gp.small_back) {               // small maps (sl2_small.hip): the search kernel alone, scoring is the back's
        if ((q = launch_search_kernel(g)) != SL2_OK) return q;
        return launch_small_back(g, gp.save_trajectory, gp.panel_w);
      }
      if ((q = launch_search(g)) != SL2_OK) return q;
      if ((q = launch_update(g)) != SL2_OK) return q;
      return launch_finalize(g, gp.save_trajectory);
    });
    if (r == SL2_OK && plan.tail.runs) r = launch_mapping(mapping_group(e), plan.tail);
    return r;
  };
  // Whole-step HIP graph: the dozen launches of a step are captured once per (frame buffer, step plan) and replayed -
  // at small batches the step is launch-bound.  Needs device-resident frames (the capture bakes the pointer in; a
  // double-buffered ingest alternates between two graphs), one sequence group and no per-kernel profiling.
  const bool use_graph = e->graph_mode && frames_on_device && !e->profiling && e->groups.size() <= 1;
  if (use_graph) {
    hipGraphExec_t exec = nullptr;
    for (const auto& sg : e->step_graphs)
      if (sg.frames == (const void*)frames && sg.stride == seq_stride && sg.plan == plan) { exec = sg.exec; break; }
    if (!exec) {
      hipGraph_t graph = nullptr;
      SL2_HIP(hipStreamBeginCapture(e->stream, hipStreamCaptureModeRelaxed));
      rc = issue();
      const hipError_t ce = hipStreamEndCapture(e->stream, &graph);     // always: a stream left capturing is unusable
      if (rc != SL2_OK || ce != hipSuccess) {
        if (graph) hipGraphDestroy(graph);
        (void)hipGetLastError();                                        // clear the sticky capture error
        if (rc != SL2_OK) return rc;
        SL2_HIP(ce);
      }
      SL2_HIP(hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0));
      e->graph_captures += 1;
      hipGraphDestroy(graph);
      if (e->step_graphs.size() >= 8) { hipGraphExecDestroy(e->step_graphs.front().exec); e->step_graphs.erase(e->step_graphs.begin()); }
      e->step_graphs.push_back({(const void*)frames, seq_stride, plan, exec});
    }
    SL2_HIP(hipGraphLaunch(exec, e->stream));
    rc = SL2_OK;
  } else {
    rc = issue();
  }
  if (rc != SL2_OK) return rc;
  e->steps_done += 1;
  if (e->profiling && e->pending.size() > 8192) return e->fold_events();
  return SL2_OK;
}

int sl2_set_graph_mode(sl2_engine* e, int enabled) {
  if (!e) return SL2_ERR_INVALID;
  SL2_HIP(hipSetDevice(e->device));
  { int _rc = drop_step_graphs(e); if (_rc != SL2_OK) return _rc; }
  e->graph_mode = enabled != 0;
  return SL2_OK;
}

// ----------------------------------------------------------------- state access

struct HostSeq {
  std::vector<double> x, P;
  std::vector<int> flags, labels, pos_err, ps;     // ps: [kpart][kPsInts]
  int n_slots = 0;
  int part[kPartInts] = {0};
  // partial slot (0 .. kpart - 1) of the partially initialised feature whose label sits in feature slot f; -1: none
  int pslot_of(int f, int kpart) const {
    for (int k = 0; k < kpart; ++k)
      if (ps[(size_t)k * kPsInts + kPsActive] && ps[(size_t)k * kPsInts + kPsLabel] == f) return k;
    return -1;
  }
};

static int fetch_seq(sl2_engine* e, int seq, bool want_P, HostSeq& hs) {
  SL2_HIP(hipSetDevice(e->device));
  { int _rc = e->sync_all(); if (_rc != SL2_OK) return _rc; }
  SL2_HIP(hipMemcpy(&hs.n_slots, e->n_slots + seq, sizeof(int), hipMemcpyDeviceToHost));
  SL2_HIP(hipMemcpy(hs.part, e->part_i + (size_t)seq * kPartInts, sizeof(int) * kPartInts, hipMemcpyDeviceToHost));
  hs.flags.resize(e->N);
  SL2_HIP(hipMemcpy(hs.flags.data(), e->f_flags + (size_t)seq * e->N, sizeof(int) * e->N, hipMemcpyDeviceToHost));
  hs.labels.resize(e->N);
  SL2_HIP(hipMemcpy(hs.labels.data(), e->f_label + (size_t)seq * e->N, sizeof(int) * e->N, hipMemcpyDeviceToHost));
  hs.pos_err.resize(e->N);
  SL2_HIP(hipMemcpy(hs.pos_err.data(), e->pos_err + (size_t)seq * e->N, sizeof(int) * e->N, hipMemcpyDeviceToHost));
  hs.ps.resize((size_t)e->kpart * kPsInts);
  SL2_HIP(hipMemcpy(hs.ps.data(), e->ps_i + (size_t)seq * e->kpart * kPsInts, sizeof(int) * hs.ps.size(), hipMemcpyDeviceToHost));
  hs.x.resize(e->ld);
  SL2_HIP(hipMemcpy(hs.x.data(), e->x + (size_t)seq * e->ld, sizeof(double) * e->ld, hipMemcpyDeviceToHost));
  if (want_P) {
    hs.P.resize((size_t)e->ld * e->ld);
    SL2_HIP(hipMemcpy(hs.P.data(), e->P + (size_t)seq * e->ld * e->ld, sizeof(double) * e->ld * e->ld, hipMemcpyDeviceToHost));
  }
  return SL2_OK;
}

// Slot that holds the feature with this label (labels are handed out once, next_free_label_++; slots are squeezed when a
// sequence runs out of them, so slot != label in general): -1 if there is none.  Synchronises.
static int slot_of_label(sl2_engine* e, int seq, int label, int* slot) {
  *slot = -1;
  { int _rc = e->sync_all(); if (_rc != SL2_OK) return _rc; }
  int ns = 0;
  SL2_HIP(hipMemcpy(&ns, e->n_slots + seq, sizeof(int), hipMemcpyDeviceToHost));
  if (ns <= 0) return SL2_OK;
  std::vector<int> lab(ns), fl(ns);
  SL2_HIP(hipMemcpy(lab.data(), e->f_label + (size_t)seq * e->N, sizeof(int) * ns, hipMemcpyDeviceToHost));
  SL2_HIP(hipMemcpy(fl.data(), e->f_flags + (size_t)seq * e->N, sizeof(int) * ns, hipMemcpyDeviceToHost));
  for (int f = 0; f < ns; ++f)
    if ((fl[f] & FF_USED) && lab[f] == label) { *slot = f; break; }
  return SL2_OK;
}

// dense index list of the live state entries (deleted features removed)
static std::vector<int> live_index(const sl2_engine* e, const HostSeq& hs) {
  std::vector<int> idx;
  for (int i = 0; i < 13; ++i) idx.push_back(i);
  for (int f = 0; f < hs.n_slots; ++f) {
    if (hs.flags[f] & FF_ACTIVE) for (int k = 0; k < 3; ++k) idx.push_back(13 + 3 * f + k);
    // a partially initialised feature sits at its label's place in feature_list_ with six states
    if (hs.flags[f] & FF_PARTIAL) {
      const int ks = hs.pslot_of(f, e->kpart);
      if (ks >= 0) for (int k = 0; k < 6; ++k) idx.push_back(e->ppos + 6 * ks + k);
    }
  }
  return idx;
}

int sl2_get_total_state_sizes(sl2_engine* e, int seq0, int nseq, int32_t* sizes) {
  if (!range_ok(e, seq0, nseq) || !sizes) return SL2_ERR_INVALID;
  SL2_HIP(hipSetDevice(e->device));
  { int _rc = e->sync_all(); if (_rc != SL2_OK) return _rc; }
  std::vector<int> flags((size_t)nseq * e->N), slots(nseq);
  SL2_HIP(hipMemcpy(flags.data(), e->f_flags + (size_t)seq0 * e->N, sizeof(int) * flags.size(), hipMemcpyDeviceToHost));
  SL2_HIP(hipMemcpy(slots.data(), e->n_slots + seq0, sizeof(int) * nseq, hipMemcpyDeviceToHost));
  for (int s = 0; s < nseq; ++s) {
    int n = 13;
    for (int f = 0; f < slots[s]; ++f) {
      if (flags[(size_t)s * e->N + f] & FF_ACTIVE) n += 3;
      if (flags[(size_t)s * e->N + f] & FF_PARTIAL) n += 6;
    }
    sizes[s] = n;
  }
  return SL2_OK;
}

int sl2_get_total_state(sl2_engine* e, int seq, double* x, int capacity) {
  if (!range_ok(e, seq, 1) || !x) return SL2_ERR_INVALID;
  HostSeq hs;
  int rc = fetch_seq(e, seq, false, hs);
  if (rc != SL2_OK) return rc;
  const std::vector<int> idx = live_index(e, hs);
  if ((int)idx.size() > capacity) return SL2_ERR_CAPACITY;
  for (size_t i = 0; i < idx.size(); ++i) x[i] = hs.x[idx[i]];
  return SL2_OK;
}

int sl2_get_total_covariance(sl2_engine* e, int seq, double* P, int capacity_n) {
  if (!range_ok(e, seq, 1) || !P) return SL2_ERR_INVALID;
  HostSeq hs;
  int rc = fetch_seq(e, seq, true, hs);
  if (rc != SL2_OK) return rc;
  const std::vector<int> idx = live_index(e, hs);
  const int n = (int)idx.size();
  if (n > capacity_n) return SL2_ERR_CAPACITY;
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) P[(size_t)i * n + j] = hs.P[(size_t)idx[i] * e->ld + idx[j]];
  return SL2_OK;
}

int sl2_get_features(sl2_engine* e, int seq, sl2_feature_info* out, int capacity, int include_deleted, int* count) {
  if (!range_ok(e, seq, 1) || !out || !count) return SL2_ERR_INVALID;
  HostSeq hs;
  int rc = fetch_seq(e, seq, false, hs);
  if (rc != SL2_OK) return rc;
  const size_t N = e->N, o = (size_t)seq * N;
  std::vector<double> h, z, nu, R, S, Hx, Hy, xo;
  std::vector<int> att, suc;
  if ((rc = fetch_vec(h, e->f_h, o * 2, N * 2))) return rc;
  if ((rc = fetch_vec(z, e->f_z, o * 2, N * 2))) return rc;
  if ((rc = fetch_vec(nu, e->f_nu, o * 2, N * 2))) return rc;
  if ((rc = fetch_vec(R, e->f_R, o, N))) return rc;
  if ((rc = fetch_vec(S, e->f_S, o * 4, N * 4))) return rc;
  if ((rc = fetch_vec(Hx, e->f_Hx, o * 14, N * 14))) return rc;
  if ((rc = fetch_vec(Hy, e->f_Hy, o * 6, N * 6))) return rc;
  if ((rc = fetch_vec(xo, e->xp_org, o * 8, N * 8))) return rc;
  if ((rc = fetch_vec(att, e->attempted, o, N))) return rc;
  if ((rc = fetch_vec(suc, e->successful, o, N))) return rc;
  int n = 0, pos = 13;
  for (int f = 0; f < hs.n_slots; ++f) {
    const int fl = hs.flags[f];
    const bool partial = fl & FF_PARTIAL;
    const bool active = (fl & FF_ACTIVE) || partial;
    if (!active && !include_deleted) continue;
    if (n >= capacity) return SL2_ERR_CAPACITY;
    sl2_feature_info& fi = out[n++];
    memset(&fi, 0, sizeof(fi));
    fi.label = hs.labels[f];
    fi.active = active ? 1 : 0;
    fi.selected_flag = (fl & FF_SELECTED) ? 1 : 0;
    fi.successful_measurement_flag = (fl & FF_SUCCESS) ? 1 : 0;
    fi.visible = (fl & FF_VISIBLE) ? 1 : 0;
    fi.attempted_measurements_of_feature = att[f];
    fi.successful_measurements_of_feature = suc[f];
    fi.position_in_total_state_vector = active ? pos - hs.pos_err[f] : -1;      // (Q28: what the reference has on record)
    fi.fully_initialised_flag = partial ? 0 : 1;
    fi.state_size = partial ? 6 : 3;
    if (active) pos += fi.state_size;
    const int pcol = partial ? e->ppos + 6 * (hs.pslot_of(f, e->kpart) < 0 ? 0 : hs.pslot_of(f, e->kpart)) : 0;
    for (int k = 0; k < 3; ++k) fi.y[k] = partial ? hs.x[pcol + k] : hs.x[13 + 3 * f + k];
    for (int k = 0; k < 3; ++k) fi.y_direction[k] = partial ? hs.x[pcol + 3 + k] : 0.0;
    for (int k = 0; k < 2; ++k) { fi.h[k] = h[f * 2 + k]; fi.z[k] = z[f * 2 + k]; fi.nu[k] = nu[f * 2 + k]; }
    fi.R = R[f];
    for (int k = 0; k < 4; ++k) fi.S[k] = S[f * 4 + k];
    for (int k = 0; k < 14; ++k) fi.dh_by_dxp[k] = Hx[f * 14 + k];
    for (int k = 0; k < 6; ++k) fi.dh_by_dy[k] = Hy[f * 6 + k];
    for (int k = 0; k < 7; ++k) fi.xp_org[k] = xo[f * 8 + k];
  }
  *count = n;
  return SL2_OK;
}

int sl2_get_partial_feature(sl2_engine* e, int seq, int index, int32_t* ints, double* dbl, double* particles, int capacity) {
  if (!range_ok(e, seq, 1) || !ints || !dbl || index < 0) return SL2_ERR_INVALID;
  SL2_HIP(hipSetDevice(e->device));
  { int _rc = e->sync_all(); if (_rc != SL2_OK) return _rc; }
  int pi[kPartInts];
  double pd[kPartDoubles];
  SL2_HIP(hipMemcpy(pi, e->part_i + (size_t)seq * kPartInts, sizeof(pi), hipMemcpyDeviceToHost));
  SL2_HIP(hipMemcpy(pd, e->part_d + (size_t)seq * kPartDoubles, sizeof(pd), hipMemcpyDeviceToHost));
  for (int k = 0; k < 16; ++k) ints[k] = 0;
  for (int k = 0; k < 9; ++k) dbl[k] = 0.0;
  const int count = pi[kPartCount];
  ints[0] = count;
  ints[5] = pi[kPartUU]; ints[6] = pi[kPartVV]; ints[7] = pi[kPartRegionValid];
  for (int k = 0; k < 4; ++k) ints[8 + k] = pi[kPartRegion + k];
  ints[12] = pi[kPartInitialised]; ints[13] = pi[kPartConverted]; ints[14] = pi[kPartDeleted]; ints[15] = pi[kPartCreated];
  dbl[8] = pd[2];
  if (index >= count) return SL2_OK;
  const int ks = pi[kPartOrder + index];           // the partial slot of the index-th entry of feature_init_info_vector_
  int ps[kPsInts];
  double psd[kPsDoubles];
  SL2_HIP(hipMemcpy(ps, e->ps_i + ((size_t)seq * e->kpart + ks) * kPsInts, sizeof(ps), hipMemcpyDeviceToHost));
  SL2_HIP(hipMemcpy(psd, e->ps_d + ((size_t)seq * e->kpart + ks) * kPsDoubles, sizeof(psd), hipMemcpyDeviceToHost));
  ints[1] = -1;
  if (ps[kPsLabel] >= 0 && ps[kPsLabel] < e->N)     // the record holds the SLOT: report the label
    SL2_HIP(hipMemcpy(&ints[1], e->f_label + (size_t)seq * e->N + ps[kPsLabel], sizeof(int), hipMemcpyDeviceToHost));
  ints[2] = ps[kPsAttempts]; ints[3] = ps[kPsNp]; ints[4] = ps[kPsMaking];
  dbl[0] = psd[0]; dbl[1] = psd[1];
  SL2_HIP(hipMemcpy(dbl + 2, e->x + (size_t)seq * e->ld + e->ppos + 6 * ks, sizeof(double) * 6, hipMemcpyDeviceToHost));
  if (particles) {
    const int n = ps[kPsNp] < capacity ? ps[kPsNp] : capacity;
    if (n > 0)
      SL2_HIP(hipMemcpy(particles, e->particles + ((size_t)seq * e->kpart + ks) * e->pcap * kParticleDoubles,
                        sizeof(double) * n * kParticleDoubles, hipMemcpyDeviceToHost));
  }
  return SL2_OK;
}

int sl2_get_selection(sl2_engine* e, int seq, int32_t* labels, int capacity, int32_t counters[3]) {
  if (!range_ok(e, seq, 1) || !labels || !counters) return SL2_ERR_INVALID;
  SL2_HIP(hipSetDevice(e->device));
  { int _rc = e->sync_all(); if (_rc != SL2_OK) return _rc; }
  int ns = 0, nv = 0, mc = 0;
  SL2_HIP(hipMemcpy(&ns, e->n_sel + seq, sizeof(int), hipMemcpyDeviceToHost));
  SL2_HIP(hipMemcpy(&nv, e->n_vis + seq, sizeof(int), hipMemcpyDeviceToHost));
  SL2_HIP(hipMemcpy(&mc, e->m_count + seq, sizeof(int), hipMemcpyDeviceToHost));
  if (ns > capacity) return SL2_ERR_CAPACITY;
  // delete_feature() deselects the feature it removes (monoslam.cpp:800-801): features deleted at
  // the end of the step no longer appear in selected_feature_list_
  std::vector<int> sel(ns > 0 ? ns : 1), flags(e->N), lab(e->N);
  if (ns > 0) SL2_HIP(hipMemcpy(sel.data(), e->sel_idx + (size_t)seq * e->N, sizeof(int) * ns, hipMemcpyDeviceToHost));
  SL2_HIP(hipMemcpy(flags.data(), e->f_flags + (size_t)seq * e->N, sizeof(int) * e->N, hipMemcpyDeviceToHost));
  SL2_HIP(hipMemcpy(lab.data(), e->f_label + (size_t)seq * e->N, sizeof(int) * e->N, hipMemcpyDeviceToHost));
  int kept = 0;
  for (int k = 0; k < ns; ++k)
    if (sel[k] >= 0 && (flags[sel[k]] & FF_ACTIVE)) labels[kept++] = lab[sel[k]];
  counters[0] = nv; counters[1] = kept; counters[2] = 2 * mc;
  return SL2_OK;
}

int sl2_get_feature_patch(sl2_engine* e, int seq, int label, uint8_t* patch121) {
  if (!range_ok(e, seq, 1) || !patch121 || label < 0) return SL2_ERR_INVALID;
  SL2_HIP(hipSetDevice(e->device));
  int slot = -1;
  { int _rc = slot_of_label(e, seq, label, &slot); if (_rc != SL2_OK) return _rc; }
  if (slot < 0) { set_error("sl2_get_feature_patch: no feature with this label"); return SL2_ERR_INVALID; }
  SL2_HIP(hipMemcpy(patch121, e->patch + ((size_t)seq * e->N + slot) * kPatchStride, SL2_PATCH_BYTES, hipMemcpyDeviceToHost));
  return SL2_OK;
}

// MonoSLAM::SavePatch (monoslam.cpp:1551-1572): cv::imwrite("patch.png", patch_) of the marked feature.  The file type
// follows the extension like cv::imwrite: ".pgm" = binary PGM, anything else = 8-bit greyscale PNG (stored with zlib).
int sl2_save_patch(sl2_engine* e, int seq, int label, const char* path) {
  if (!path) return SL2_ERR_INVALID;
  uint8_t patch[SL2_PATCH_BYTES];
  int rc = sl2_get_feature_patch(e, seq, label, patch);
  if (rc != SL2_OK) return rc;
  return write_grey_image(path, patch, SL2_PATCH_SIZE, SL2_PATCH_SIZE);
}

int sl2_get_trajectory(sl2_engine* e, int seq, double* out, int capacity, int* count) {
  if (!range_ok(e, seq, 1) || !out || !count) return SL2_ERR_INVALID;
  SL2_HIP(hipSetDevice(e->device));
  { int _rc = e->sync_all(); if (_rc != SL2_OK) return _rc; }
  int total = 0;
  SL2_HIP(hipMemcpy(&total, e->traj_count + seq, sizeof(int), hipMemcpyDeviceToHost));
  std::vector<double> ring((size_t)kTrajCapacity * 3);
  SL2_HIP(hipMemcpy(ring.data(), e->traj + (size_t)seq * kTrajCapacity * 3, sizeof(double) * ring.size(), hipMemcpyDeviceToHost));
  int have = total < kTrajCapacity ? total : kTrajCapacity;
  int n = have < capacity ? have : capacity;
  // oldest-first among the n most recent
  for (int i = 0; i < n; ++i) {
    const int logical = total - n + i;
    const int slot = logical % kTrajCapacity;
    for (int k = 0; k < 3; ++k) out[i * 3 + k] = ring[(size_t)slot * 3 + k];
  }
  *count = n;
  return SL2_OK;
}

int sl2_get_position_log(sl2_engine* e, int seq0, int nseq, double* out, int capacity, int* count) {
  if (!range_ok(e, seq0, nseq) || !out || !count || capacity <= 0) return SL2_ERR_INVALID;
  SL2_HIP(hipSetDevice(e->device));
  { int _rc = e->sync_all(); if (_rc != SL2_OK) return _rc; }
  const long long total = e->steps_done;
  const int have = (int)(total < kTrajCapacity ? total : kTrajCapacity);
  const int n = have < capacity ? have : capacity;
  std::vector<double> ring((size_t)nseq * kTrajCapacity * 3);
  SL2_HIP(hipMemcpy(ring.data(), e->pos_log + (size_t)seq0 * kTrajCapacity * 3, sizeof(double) * ring.size(), hipMemcpyDeviceToHost));
  for (int s = 0; s < nseq; ++s)
    for (int i = 0; i < n; ++i) {
      const int slot = (int)((total - n + i) % kTrajCapacity);
      for (int k = 0; k < 3; ++k) out[((size_t)s * n + i) * 3 + k] = ring[((size_t)s * kTrajCapacity + slot) * 3 + k];
    }
  *count = n;
  return SL2_OK;
}

#ifdef SL2_TESTING   // test hook: libscenelib2_amd_test.so only (include/scenelib2_amd_testing.h)
int sl2_debug_graph_captures(sl2_engine* e) { return e ? (int)e->graph_captures : -1; }

// One sequence's covariance as the kernels hold it: all ld rows of ld doubles, padding and never-used slots included.
int sl2_debug_raw_covariance(sl2_engine* e, int seq, double* P, int capacity_ld, int* ld) {
  if (!range_ok(e, seq, 1) || !P || !ld) return SL2_ERR_INVALID;
  *ld = e->ld;
  if (e->ld > capacity_ld) return SL2_ERR_CAPACITY;
  SL2_HIP(hipSetDevice(e->device));
  { int _rc = e->sync_all(); if (_rc != SL2_OK) return _rc; }
  SL2_HIP(hipMemcpy(P, e->P + (size_t)seq * e->ld * e->ld, sizeof(double) * e->ld * e->ld, hipMemcpyDeviceToHost));
  return SL2_OK;
}

int sl2_set_feature_counters(sl2_engine* e, int seq, int label, int attempted, int successful) {
  if (!range_ok(e, seq, 1) || label < 0) return SL2_ERR_INVALID;
  SL2_HIP(hipSetDevice(e->device));
  int slot = -1;
  { int _rc = slot_of_label(e, seq, label, &slot); if (_rc != SL2_OK) return _rc; }
  if (slot < 0) return SL2_ERR_INVALID;
  SL2_HIP(hipMemcpy(e->attempted + (size_t)seq * e->N + slot, &attempted, sizeof(int), hipMemcpyHostToDevice));
  SL2_HIP(hipMemcpy(e->successful + (size_t)seq * e->N + slot, &successful, sizeof(int), hipMemcpyHostToDevice));
  return SL2_OK;
}
// How far the RECORDED position_in_total_state_vector_ of a feature lies below its true one (Q28, feature.cpp:254), written
// directly: several conversions' worth of error without running them.
int sl2_debug_set_position_error(sl2_engine* e, int seq, int label, int err) {
  if (!range_ok(e, seq, 1) || label < 0 || err < 0 || err % 3) return SL2_ERR_INVALID;
  SL2_HIP(hipSetDevice(e->device));
  int slot = -1;
  { int _rc = slot_of_label(e, seq, label, &slot); if (_rc != SL2_OK) return _rc; }
  if (slot < 0) return SL2_ERR_INVALID;
  const int one = 1;
  SL2_HIP(hipMemcpy(e->pos_err + (size_t)seq * e->N + slot, &err, sizeof(int), hipMemcpyHostToDevice));
  if (err) SL2_HIP(hipMemcpy(e->pos_err_any + seq, &one, sizeof(int), hipMemcpyHostToDevice));
  return SL2_OK;
}
#endif  // SL2_TESTING

// mark_feature_by_lab + delete_feature for one feature per sequence (monoslam.cpp:743-812): the slot is retired
// (inactive, deselected, its label never reused) and its rows / columns of P are zeroed, which is what removing them from
// the total state amounts to in this layout (k_finalize does the same for delete_bad_features).
__global__ void __launch_bounds__(256) k_delete_feature(double* __restrict__ P, int* __restrict__ f_flags, const int* __restrict__ f_label,
                                                        const int* __restrict__ n_slots, const int* __restrict__ labels,
                                                        int* __restrict__ done, int N, int ld) {
  const int b = blockIdx.x;
  const int lab = labels[b];
  __shared__ int s_slot;
  if (threadIdx.x == 0) s_slot = -1;
  __syncthreads();
  if (lab >= 0)
    for (int f = threadIdx.x; f < n_slots[b]; f += blockDim.x) {
      const int fl = f_flags[(size_t)b * N + f];
      if ((fl & FF_ACTIVE) && !(fl & FF_PARTIAL) && f_label[(size_t)b * N + f] == lab) s_slot = f;    // labels are unique
    }
  __syncthreads();
  const int slot = s_slot;
  const bool ok = slot >= 0;
  if (threadIdx.x == 0) { done[b] = ok ? 1 : 0; if (ok) f_flags[(size_t)b * N + slot] = FF_USED; }
  if (!ok) return;
  double* Pb = P + (size_t)b * ld * ld;
  const int pos = 13 + 3 * slot;
  for (int j = threadIdx.x; j < ld; j += blockDim.x)
    for (int r = 0; r < 3; ++r) {
      Pb[(size_t)(pos + r) * ld + j] = 0.0;
      Pb[(size_t)j * ld + pos + r] = 0.0;
    }
}

int sl2_delete_features(sl2_engine* e, int seq0, int nseq, const int32_t* labels, int32_t* deleted) {
  if (!range_ok(e, seq0, nseq) || !labels) return SL2_ERR_INVALID;
  SL2_HIP(hipSetDevice(e->device));
  { int _rc = e->sync_all(); if (_rc != SL2_OK) return _rc; }
  e->parts_block_step = e->steps_done;       // (nothing here touches a partial feature today; the next step takes no shortcut all the same)
  int *d_lab = nullptr, *d_done = nullptr;
  SL2_HIP(hipMalloc((void**)&d_lab, sizeof(int) * nseq));
  if (hipMalloc((void**)&d_done, sizeof(int) * nseq) != hipSuccess) { hipFree(d_lab); set_error("hipMalloc failed"); return SL2_ERR_HIP; }
  hipError_t err = hipMemcpy(d_lab, labels, sizeof(int) * nseq, hipMemcpyHostToDevice);
  if (err == hipSuccess) {
    hipLaunchKernelGGL(k_delete_feature, dim3(nseq), dim3(256), 0, e->stream, e->P + (size_t)seq0 * e->ld * e->ld,
                       e->f_flags + (size_t)seq0 * e->N, e->f_label + (size_t)seq0 * e->N, e->n_slots + seq0, d_lab, d_done,
                       e->N, e->ld);
    err = hipGetLastError();
  }
  if (err == hipSuccess) err = hipStreamSynchronize(e->stream);
  std::vector<int32_t> done(nseq, 0);
  if (err == hipSuccess) err = hipMemcpy(done.data(), d_done, sizeof(int) * nseq, hipMemcpyDeviceToHost);
  hipFree(d_lab); hipFree(d_done);
  if (err != hipSuccess) { set_error(hipGetErrorString(err)); return SL2_ERR_HIP; }
  if (deleted) for (int i = 0; i < nseq; ++i) deleted[i] = done[i];
  return SL2_OK;
}

int sl2_get_status_flags(sl2_engine* e, int seq0, int nseq, int32_t* flags) {
  if (!range_ok(e, seq0, nseq) || !flags) return SL2_ERR_INVALID;
  SL2_HIP(hipSetDevice(e->device));
  { int _rc = e->sync_all(); if (_rc != SL2_OK) return _rc; }
  SL2_HIP(hipMemcpy(flags, e->status + seq0, sizeof(int) * nseq, hipMemcpyDeviceToHost));
  return SL2_OK;
}

// ------------------------------------------------------------------- profiling

int sl2_set_profiling(sl2_engine* e, int enabled) {
  if (!e) return SL2_ERR_INVALID;
  if (!enabled && e->profiling) { int rc = e->fold_events(); if (rc) return rc; }
  e->profiling = enabled != 0;
  if (enabled) e->profile_level = enabled >= 2 ? 2 : 1;
  return SL2_OK;
}
int sl2_set_profile_focus(sl2_engine* e, const char* names) {
  if (!e) return SL2_ERR_INVALID;
  e->profile_focus = (names && *names) ? std::string(",") + names + "," : std::string();
  return SL2_OK;
}
int sl2_reset_kernel_times(sl2_engine* e) {
  if (!e) return SL2_ERR_INVALID;
  int rc = e->fold_events();
  if (rc) return rc;
  for (auto& t : e->timers) { t.total_ms = 0; t.launches = 0; }
  return SL2_OK;
}
int sl2_kernel_count(sl2_engine* e) {
  if (!e) return 0;
  e->fold_events();
  return (int)e->timers.size();
}
int sl2_get_kernel_time(sl2_engine* e, int idx, const char** name, double* total_ms, int64_t* launches) {
  if (!e || idx < 0 || idx >= (int)e->timers.size()) return SL2_ERR_INVALID;
  int rc = e->fold_events();
  if (rc) return rc;
  if (name) *name = e->timers[idx].name.c_str();
  if (total_ms) *total_ms = e->timers[idx].total_ms;
  if (launches) *launches = e->timers[idx].launches;
  return SL2_OK;
}

int sl2_get_placement(sl2_engine* e, double* out, int capacity) {
  if (!e || !out || capacity < 0) return SL2_ERR_INVALID;
  const sl2_engine* r = e->root;
  const double v[SL2_PLACEMENT_COUNT] = {(double)r->place_candidates, r->place_kept_ms[0], r->place_kept_ms[1], r->place_kept_ms[2],
                                         r->place_kept_ms[3], r->place_worst_ms[0], r->place_worst_ms[1], r->place_worst_ms[2],
                                         r->place_syrk_ms[0], r->place_syrk_ms[1]};
  for (int i = 0; i < capacity && i < SL2_PLACEMENT_COUNT; ++i) out[i] = v[i];
  return SL2_OK;
}

int sl2_get_step_work(sl2_engine* e, double* out_caller, int capacity) {
  if (!e || !out_caller || capacity < 1) return SL2_ERR_INVALID;
  double out[SL2_STEP_WORK_COUNT];
  SL2_HIP(hipSetDevice(e->device));
  { int _rc = e->sync_all(); if (_rc != SL2_OK) return _rc; }
  std::vector<double> w((size_t)e->B * kWorkDoubles);
  std::vector<int> mc(e->B), flags((size_t)e->B * e->N), slots(e->B);
  std::vector<uint8_t> act(e->B);
  SL2_HIP(hipMemcpy(act.data(), e->active, (size_t)e->B, hipMemcpyDeviceToHost));
  SL2_HIP(hipMemcpy(w.data(), e->work, sizeof(double) * w.size(), hipMemcpyDeviceToHost));
  SL2_HIP(hipMemcpy(mc.data(), e->m_count, sizeof(int) * e->B, hipMemcpyDeviceToHost));
  SL2_HIP(hipMemcpy(flags.data(), e->f_flags, sizeof(int) * flags.size(), hipMemcpyDeviceToHost));
  SL2_HIP(hipMemcpy(slots.data(), e->n_slots, sizeof(int) * e->B, hipMemcpyDeviceToHost));
  for (int k = 0; k < SL2_STEP_WORK_COUNT; ++k) out[k] = 0.0;
  const double frame_bytes = (double)e->cam.width * e->cam.height;
  for (int b = 0; b < e->B; ++b) {
    if (!act[b]) continue;                  // a paused sequence did no work in the step (its counters are those of the last frame it saw)
    const double win = w[(size_t)b * kWorkDoubles + 0];
    out[0] += win < frame_bytes ? win : frame_bytes;
    out[1] += w[(size_t)b * kWorkDoubles + 1];
    out[2] += w[(size_t)b * kWorkDoubles + 2];
    out[10] += w[(size_t)b * kWorkDoubles + 3];
    out[11] += w[(size_t)b * kWorkDoubles + 4];
    double n = 13;
    for (int f = 0; f < slots[b]; ++f) if (flags[(size_t)b * e->N + f] & FF_ACTIVE) n += 3;
    const double m = 2.0 * mc[b];
    out[3] += m; out[4] += m * m; out[5] += m * m * m; out[6] += n; out[7] += n * m; out[8] += n * n * m; out[9] += n * m * m;
  }
  for (sl2_engine* g : e->groups)
    if (g->srch_big) {
      int last = 0;
      SL2_HIP(hipMemcpy(&last, g->srch_big + 1, sizeof(int), hipMemcpyDeviceToHost));     // (k_search_score leaves the step's count there)
      out[12] += last;
    }
  for (int k = 0; k < capacity && k < SL2_STEP_WORK_COUNT; ++k) out_caller[k] = out[k];   // never beyond the caller's array
  return SL2_OK;
}

// ------------------------------------------------------ device-memory helpers

int sl2_dev_malloc(int device, size_t bytes, void** out) {
  if (!out) return SL2_ERR_INVALID;
  int rc = check_device();
  if (rc) return rc;
  SL2_HIP(hipSetDevice(device));
  SL2_HIP(hipMalloc(out, bytes ? bytes : 1));
  return SL2_OK;
}
int sl2_dev_free(int device, void* p) {
  SL2_HIP(hipSetDevice(device));
  SL2_HIP(hipFree(p));
  return SL2_OK;
}
int sl2_dev_upload(int device, void* dst_dev, const void* src_host, size_t bytes) {
  SL2_HIP(hipSetDevice(device));
  SL2_HIP(hipMemcpy(dst_dev, src_host, bytes, hipMemcpyHostToDevice));
  return SL2_OK;
}
int sl2_dev_download(int device, void* dst_host, const void* src_dev, size_t bytes) {
  SL2_HIP(hipSetDevice(device));
  SL2_HIP(hipMemcpy(dst_host, src_dev, bytes, hipMemcpyDeviceToHost));
  return SL2_OK;
}

#ifdef SL2_TESTING   // test hook: libscenelib2_amd_test.so only
int sl2_debug_ncc_score(int device, const int32_t* sums5, int count, double* score, double* sd0, double* sd1) {
  if (!sums5 || !score || !sd0 || !sd1 || count <= 0) return SL2_ERR_INVALID;
  int rc = check_device();
  if (rc) return rc;
  SL2_HIP(hipSetDevice(device));
  int* ds = nullptr;
  double *dsc = nullptr, *d0 = nullptr, *d1 = nullptr;
  SL2_HIP(hipMalloc(&ds, sizeof(int) * 5 * count));
  SL2_HIP(hipMalloc(&dsc, sizeof(double) * count));
  SL2_HIP(hipMalloc(&d0, sizeof(double) * count));
  SL2_HIP(hipMalloc(&d1, sizeof(double) * count));
  SL2_HIP(hipMemcpy(ds, sums5, sizeof(int) * 5 * count, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_ncc_score, dim3((count + 255) / 256), dim3(256), 0, 0, ds, count, dsc, d0, d1);
  SL2_HIP(hipGetLastError());
  SL2_HIP(hipDeviceSynchronize());
  SL2_HIP(hipMemcpy(score, dsc, sizeof(double) * count, hipMemcpyDeviceToHost));
  SL2_HIP(hipMemcpy(sd0, d0, sizeof(double) * count, hipMemcpyDeviceToHost));
  SL2_HIP(hipMemcpy(sd1, d1, sizeof(double) * count, hipMemcpyDeviceToHost));
  hipFree(ds); hipFree(dsc); hipFree(d0); hipFree(d1);
  return SL2_OK;
}
#endif  // SL2_TESTING

}  // extern "C"

namespace sl2 {
int checkpoint_refresh_slots(sl2_engine* e) { return refresh_slots_exact(e); }
int checkpoint_drop_graphs(sl2_engine* e) { return drop_step_graphs(e); }
int checkpoint_enable_mapping(sl2_engine* e) { return enable_feature_initialisation(e); }
}  // namespace sl2
