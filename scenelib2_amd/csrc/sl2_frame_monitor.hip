// The frame monitor (include/scenelib2_amd.h, "the frame monitor").
//
// k_frame_stats: a streaming read of the batch's frames.  A workgroup of kFrameThreads threads owns one sequence (grid.x: batches
// above 65 535 sequences) and one band of rows (grid.y).  A frame is one run of n = W * H bytes, and a band of a multiple of 16 rows
// starts on a multiple of 16 bytes, so a band is a whole number of 16-byte chunks (the frame's last chunk may be short) and a
// lane takes one chunk per pass: one 16-byte load where the frame's address is a multiple of 16, sixteen byte loads elsewhere -
// the arithmetic (frame_chunk_accumulate, sl2_frame_monitor_dev.hpp) is the same.  The chunks above and below it, which the
// gradient needs, are 16-byte loads too where the width is a multiple of 16 and byte loads elsewhere; they belong to the
// neighbouring rows and hit the caches.  Every accumulator is a register of the lane (the histogram: sixteen counters fed from
// two words of 4-bit fields per chunk); they are summed across the wave by shuffles and across the four waves by LDS integer
// atomics, and the workgroup writes ONE partial record with plain stores.  No workgroup waits for another.
//
// k_frame_gate: one wave per sequence sums the band partials in band order (integer sums, minima and maxima: the order does not
// matter to the value, and it is fixed anyway), writes the record, applies the gate (frame_verdict), writes the verdict and the
// active byte and stores the digest for the next examination.
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../../include/scenelib2_amd_testing.h"
#include "sl2_common.hpp"
#include "sl2_frame_monitor_dev.hpp"

static_assert(sizeof(sl2_frame_stats) == 104 && sizeof(sl2_frame_gate) == 32, "the layouts of scenelib2_amd.h");
static_assert(SL2_FRAME_MONITOR_BAND_ROWS == sl2::kFrameBandRows, "scenelib2_amd_testing.h repeats the band height for the tests");

namespace sl2 {

struct FrameStatsArgs {
  const uint8_t* frames;
  size_t seq_stride;
  const uint8_t* base_active;      // or nullptr
  sl2_frame_stats* partials;       // [batch][bands]
  int W, H, band_rows, bands;
};

// Bytes [off, off + 16) of the frame: one load where VEC says such offsets are 16-byte addresses and the chunk lies whole in the frame
template <bool VEC>
__device__ __forceinline__ FrameChunk frame_load(const uint8_t* __restrict__ f, int64_t off, int64_t n) {
  if (VEC && off >= 0 && off + kFrameChunk <= n) {
    const uint4 v = *reinterpret_cast<const uint4*>(f + off);
    FrameChunk c;
    c.w[0] = v.x; c.w[1] = v.y; c.w[2] = v.z; c.w[3] = v.w;
    return c;
  }
  return frame_load_bytes(f, off, n);
}

// The lane's chunks of the band [c0, c1): VEC = the frame's address is a multiple of 16, VEC_ROWS = and so is the width
template <bool VEC, bool VEC_ROWS>
__device__ __forceinline__ void frame_band(FrameAcc& a, const uint8_t* __restrict__ f, int64_t n, int W, int H, int64_t c0, int64_t c1) {
  for (int64_t c = c0 + threadIdx.x; c < c1; c += kFrameThreads) {
    const int64_t off = c * kFrameChunk;
    const int cnt = n - off < kFrameChunk ? (int)(n - off) : kFrameChunk;
    const FrameChunk self = frame_load<VEC>(f, off, n);
    const FrameChunk up = frame_load<VEC_ROWS>(f, off - W, n), down = frame_load<VEC_ROWS>(f, off + W, n);
    const int left = off >= 1 ? f[off - 1] : 0, right = off + kFrameChunk < n ? f[off + kFrameChunk] : 0;
    frame_chunk_accumulate(a, self, left, right, up, down, c, cnt, W, H);
  }
}

__device__ __forceinline__ uint64_t wave_sum64(uint64_t v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += (uint64_t)__shfl_xor((unsigned long long)v, o, 64);
  return v;
}
__device__ __forceinline__ uint32_t wave_sum32(uint32_t v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, 64);
  return v;
}

__global__ __launch_bounds__(kFrameThreads) void k_frame_stats(FrameStatsArgs A) {
  const int b = blockIdx.x, band = blockIdx.y;
  if (A.base_active && A.base_active[b] == 0) return;          // not examined: none of its bytes are read, no partial written
  const uint8_t* __restrict__ f = A.frames + (size_t)b * A.seq_stride;
  const int64_t n = (int64_t)A.W * A.H;
  const int64_t lo = (int64_t)band * A.band_rows * A.W;        // a multiple of 16: band_rows is
  const int64_t hi = lo + (int64_t)A.band_rows * A.W < n ? lo + (int64_t)A.band_rows * A.W : n;
  const int64_t c0 = lo / kFrameChunk, c1 = frame_chunks(hi);

  __shared__ unsigned long long s_sum[4];
  __shared__ unsigned int s_mn, s_mx, s_hist[16];
  if (threadIdx.x < 4) s_sum[threadIdx.x] = 0;
  if (threadIdx.x < 16) s_hist[threadIdx.x] = 0;
  if (threadIdx.x == 0) { s_mn = 0xFFFFFFFFu; s_mx = 0; }
  __syncthreads();

  FrameAcc a;
  const bool vec = (reinterpret_cast<uintptr_t>(f) & 15u) == 0;
  if (vec && (A.W & 15) == 0) frame_band<true, true>(a, f, n, A.W, A.H, c0, c1);
  else if (vec) frame_band<true, false>(a, f, n, A.W, A.H, c0, c1);
  else frame_band<false, false>(a, f, n, A.W, A.H, c0, c1);

  // across the wave in registers, across the waves by LDS integer atomics
  a.sum = wave_sum64(a.sum); a.sum_sq = wave_sum64(a.sum_sq); a.grad = wave_sum64(a.grad); a.digest = wave_sum64(a.digest);
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const uint32_t mn = (uint32_t)__shfl_xor((int)a.mn, o, 64), mx = (uint32_t)__shfl_xor((int)a.mx, o, 64);
    a.mn = mn < a.mn ? mn : a.mn; a.mx = mx > a.mx ? mx : a.mx;
  }
#pragma unroll
  for (int j = 0; j < 16; ++j) a.hist[j] = wave_sum32(a.hist[j]);
  if ((threadIdx.x & 63) == 0) {
    atomicAdd(&s_sum[0], (unsigned long long)a.sum); atomicAdd(&s_sum[1], (unsigned long long)a.sum_sq);
    atomicAdd(&s_sum[2], (unsigned long long)a.grad); atomicAdd(&s_sum[3], (unsigned long long)a.digest);
    atomicMin(&s_mn, a.mn); atomicMax(&s_mx, a.mx);
#pragma unroll
    for (int j = 0; j < 16; ++j) atomicAdd(&s_hist[j], a.hist[j]);
  }
  __syncthreads();
  sl2_frame_stats* __restrict__ P = A.partials + ((size_t)b * A.bands + band);
  if (threadIdx.x == 0) {
    P->sum = s_sum[0]; P->sum_sq = s_sum[1]; P->gradient_energy = s_sum[2]; P->digest = s_sum[3];
    P->min = s_mn; P->max = s_mx;
  }
  if (threadIdx.x < 16) P->hist[threadIdx.x] = s_hist[threadIdx.x];
}

struct FrameGateArgs {
  const sl2_frame_stats* partials;
  int bands;
  const uint8_t* base_active;      // or nullptr
  const sl2_frame_gate* gates;     // [batch]
  uint64_t* prev_digest;           // [batch]
  uint8_t* have_prev;              // [batch]
  sl2_frame_stats* stats_mon;      // [batch]: the monitor's own copy (sl2_frame_monitor_read)
  uint32_t* verdict_mon;
  sl2_frame_stats* stats_out;      // the caller's, or nullptr
  uint32_t* verdict_out;
  uint8_t* active_out;
};

constexpr int kFrameGateThreads = 64;

__global__ __launch_bounds__(kFrameGateThreads) void k_frame_gate(FrameGateArgs A) {
  const int b = blockIdx.x, lane = threadIdx.x;
  if (A.base_active && A.base_active[b] == 0) {          // (active_out may be the same array: this block alone touches entry b)
    if (lane == 0) {
      A.verdict_mon[b] = SL2_FRAME_SKIPPED;
      if (A.verdict_out) A.verdict_out[b] = SL2_FRAME_SKIPPED;
      if (A.active_out) A.active_out[b] = 0;
    }
    return;
  }
  // one field per lane, the bands in order: lanes 0 .. 3 the 64-bit sums, 4 and 5 min and max, 6 .. 21 the histogram
  __shared__ sl2_frame_stats s;
  const sl2_frame_stats* __restrict__ P = A.partials + (size_t)b * A.bands;
  if (lane < 4) {
    uint64_t v = 0;
    for (int k = 0; k < A.bands; ++k) v += lane == 0 ? P[k].sum : lane == 1 ? P[k].sum_sq : lane == 2 ? P[k].gradient_energy : P[k].digest;
    if (lane == 0) s.sum = v; else if (lane == 1) s.sum_sq = v; else if (lane == 2) s.gradient_energy = v; else s.digest = v;
  } else if (lane == 4) {
    uint32_t v = 0xFFFFFFFFu;
    for (int k = 0; k < A.bands; ++k) v = P[k].min < v ? P[k].min : v;
    s.min = v;
  } else if (lane == 5) {
    uint32_t v = 0;
    for (int k = 0; k < A.bands; ++k) v = P[k].max > v ? P[k].max : v;
    s.max = v;
  } else if (lane < 22) {
    uint32_t v = 0;
    for (int k = 0; k < A.bands; ++k) v += P[k].hist[lane - 6];
    s.hist[lane - 6] = v;
  }
  __syncthreads();
  if (lane < (int)(sizeof(sl2_frame_stats) / 8)) {          // the record: thirteen 8-byte words
    const uint64_t w = reinterpret_cast<const uint64_t*>(&s)[lane];
    reinterpret_cast<uint64_t*>(A.stats_mon + b)[lane] = w;
    if (A.stats_out) reinterpret_cast<uint64_t*>(A.stats_out + b)[lane] = w;
  }
  if (lane == 0) {
    const uint32_t v = frame_verdict(s, A.gates[b], A.have_prev[b] != 0, A.prev_digest[b]);
    A.prev_digest[b] = s.digest; A.have_prev[b] = 1;          // whatever the verdict
    A.verdict_mon[b] = v;
    if (A.verdict_out) A.verdict_out[b] = v;
    if (A.active_out) A.active_out[b] = v == 0 ? 1 : 0;
  }
}

// The setters' changes ride in kernel arguments on the stream of the next examination: nothing to keep alive, nothing to wait for
constexpr int kFrameGateChunk = 64;
struct FrameGateChunk { sl2_frame_gate g[kFrameGateChunk]; };
__global__ void k_frame_put_gates(sl2_frame_gate* dst, FrameGateChunk c, int n) {
  const int i = threadIdx.x;
  if (i < n) dst[i] = c.g[i];
}
__global__ void k_frame_forget(uint8_t* have_prev, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) have_prev[i] = 0;
}

}  // namespace sl2

using namespace sl2;

// The opaque monitor of the C ABI
struct sl2_frame_monitor {
  int device = 0, batch = 0, W = 0, H = 0, band_rows = 0, bands = 0;
  std::vector<sl2_frame_gate> gates;          // what sl2_frame_monitor_get_gates returns
  std::vector<uint8_t> gate_dirty;            // set since the last examination
  bool any_dirty = false;
  std::vector<std::pair<int, int>> forget;    // sl2_frame_monitor_reset ranges since the last examination
  sl2_frame_stats* d_partials = nullptr;      // [batch][bands]
  sl2_frame_gate* d_gates = nullptr;
  uint64_t* d_prev = nullptr;
  uint8_t* d_have = nullptr;
  sl2_frame_stats* d_stats = nullptr;
  uint32_t* d_verdicts = nullptr;
  hipEvent_t done = nullptr;                  // the last examination queued: sl2_frame_monitor_read waits for it
  bool queued = false;
};

static bool monitor_has_range(const sl2_frame_monitor* m, int seq0, int nseq) { return seq0 >= 0 && nseq >= 0 && seq0 <= m->batch - nseq; }

extern "C" int sl2_frame_monitor_create(int device, int batch, int width, int height, sl2_frame_monitor** out) {
  if (!out || batch < 1 || !frame_size_ok(width, height)) {
    set_error("sl2_frame_monitor_create: batch >= 1, width and height >= 1 and width * height < 2^31 are required");
    return SL2_ERR_INVALID;
  }
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { set_error("no HIP device"); return SL2_ERR_NO_DEVICE; }
  if (device < 0 || device >= ndev) { set_error("sl2_frame_monitor_create: no such device"); return SL2_ERR_INVALID; }
  SL2_HIP(hipSetDevice(device));
  sl2_frame_monitor* m = new sl2_frame_monitor;
  m->device = device; m->batch = batch; m->W = width; m->H = height;
  m->band_rows = frame_band_rows(height); m->bands = frame_bands(height);
  m->gates.assign(batch, sl2_frame_gate{}); m->gate_dirty.assign(batch, 0);
  const size_t B = (size_t)batch;
  hipError_t e = hipMalloc(&m->d_partials, B * m->bands * sizeof(sl2_frame_stats));
  if (e == hipSuccess) e = hipMalloc(&m->d_gates, B * sizeof(sl2_frame_gate));
  if (e == hipSuccess) e = hipMemset(m->d_gates, 0, B * sizeof(sl2_frame_gate));
  if (e == hipSuccess) e = hipMalloc(&m->d_prev, B * sizeof(uint64_t));
  if (e == hipSuccess) e = hipMemset(m->d_prev, 0, B * sizeof(uint64_t));
  if (e == hipSuccess) e = hipMalloc(&m->d_have, B);
  if (e == hipSuccess) e = hipMemset(m->d_have, 0, B);
  if (e == hipSuccess) e = hipMalloc(&m->d_stats, B * sizeof(sl2_frame_stats));
  if (e == hipSuccess) e = hipMemset(m->d_stats, 0, B * sizeof(sl2_frame_stats));
  if (e == hipSuccess) e = hipMalloc(&m->d_verdicts, B * sizeof(uint32_t));
  if (e == hipSuccess) e = hipMemsetD32(reinterpret_cast<hipDeviceptr_t>(m->d_verdicts), SL2_FRAME_SKIPPED, B);
  if (e == hipSuccess) e = hipDeviceSynchronize();          // the fills, whatever stream the first examination uses
  if (e == hipSuccess) e = hipEventCreateWithFlags(&m->done, hipEventDisableTiming);
  if (e != hipSuccess) {
    set_error(std::string("sl2_frame_monitor_create: ") + hipGetErrorString(e));
    sl2_frame_monitor_destroy(m);
    return SL2_ERR_HIP;
  }
  *out = m;
  return SL2_OK;
}

extern "C" void sl2_frame_monitor_destroy(sl2_frame_monitor* m) {
  if (!m) return;
  hipSetDevice(m->device);
  if (m->queued) hipEventSynchronize(m->done);
  if (m->done) hipEventDestroy(m->done);
  if (m->d_partials) hipFree(m->d_partials);
  if (m->d_gates) hipFree(m->d_gates);
  if (m->d_prev) hipFree(m->d_prev);
  if (m->d_have) hipFree(m->d_have);
  if (m->d_stats) hipFree(m->d_stats);
  if (m->d_verdicts) hipFree(m->d_verdicts);
  delete m;
}

extern "C" int sl2_frame_monitor_set_gates(sl2_frame_monitor* m, int seq0, int nseq, const sl2_frame_gate* gates) {
  if (!m || !gates || !monitor_has_range(m, seq0, nseq)) { set_error("sl2_frame_monitor_set_gates: bad arguments"); return SL2_ERR_INVALID; }
  for (int i = 0; i < nseq; ++i) {
    const char* why = frame_gate_fault(gates[i]);
    if (why) {
      char buf[160];
      snprintf(buf, sizeof(buf), "sl2_frame_monitor_set_gates: sequence %d: %s", seq0 + i, why);
      set_error(buf);
      return SL2_ERR_INVALID;
    }
  }
  for (int i = 0; i < nseq; ++i) { m->gates[seq0 + i] = gates[i]; m->gate_dirty[seq0 + i] = 1; }
  if (nseq > 0) m->any_dirty = true;
  return SL2_OK;
}

extern "C" int sl2_frame_monitor_get_gates(const sl2_frame_monitor* m, int seq0, int nseq, sl2_frame_gate* gates) {
  if (!m || !gates || !monitor_has_range(m, seq0, nseq)) { set_error("sl2_frame_monitor_get_gates: bad arguments"); return SL2_ERR_INVALID; }
  for (int i = 0; i < nseq; ++i) gates[i] = m->gates[seq0 + i];
  return SL2_OK;
}

extern "C" int sl2_frame_monitor_reset(sl2_frame_monitor* m, int seq0, int nseq) {
  if (!m || !monitor_has_range(m, seq0, nseq)) { set_error("sl2_frame_monitor_reset: bad arguments"); return SL2_ERR_INVALID; }
  if (nseq > 0) m->forget.emplace_back(seq0, nseq);
  return SL2_OK;
}

extern "C" int sl2_examine_frames(sl2_frame_monitor* m, void* stream, const uint8_t* frames, size_t seq_stride, const uint8_t* base_active,
                                  sl2_frame_stats* stats_out, uint32_t* verdict_out, uint8_t* active_out) {
  if (!m || !frames) { set_error("sl2_examine_frames: bad arguments"); return SL2_ERR_INVALID; }
  if (seq_stride < (size_t)m->W * m->H) { set_error("sl2_examine_frames: seq_stride is below width * height"); return SL2_ERR_INVALID; }
  SL2_HIP(hipSetDevice(m->device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  // what the setters changed since the last examination, in front of this one
  if (m->any_dirty) {
    for (int s = 0; s < m->batch;) {
      if (!m->gate_dirty[s]) { ++s; continue; }
      FrameGateChunk c;
      int cnt = 0;
      while (s + cnt < m->batch && cnt < kFrameGateChunk && m->gate_dirty[s + cnt]) { c.g[cnt] = m->gates[s + cnt]; m->gate_dirty[s + cnt] = 0; ++cnt; }
      for (int i = cnt; i < kFrameGateChunk; ++i) c.g[i] = sl2_frame_gate{};
      hipLaunchKernelGGL(k_frame_put_gates, dim3(1), dim3(kFrameGateChunk), 0, st, m->d_gates + s, c, cnt);
      SL2_HIP(hipGetLastError());
      s += cnt;
    }
    m->any_dirty = false;
  }
  for (const auto& r : m->forget) {
    hipLaunchKernelGGL(k_frame_forget, dim3((r.second + 255) / 256), dim3(256), 0, st, m->d_have + r.first, r.second);
    SL2_HIP(hipGetLastError());
  }
  m->forget.clear();
  const FrameStatsArgs S{frames, seq_stride, base_active, m->d_partials, m->W, m->H, m->band_rows, m->bands};
  hipLaunchKernelGGL(k_frame_stats, dim3(m->batch, m->bands), dim3(kFrameThreads), 0, st, S);
  SL2_HIP(hipGetLastError());
  const FrameGateArgs G{m->d_partials, m->bands, base_active, m->d_gates, m->d_prev, m->d_have, m->d_stats, m->d_verdicts,
                        stats_out, verdict_out, active_out};
  hipLaunchKernelGGL(k_frame_gate, dim3(m->batch), dim3(kFrameGateThreads), 0, st, G);
  SL2_HIP(hipGetLastError());
  SL2_HIP(hipEventRecord(m->done, st));
  m->queued = true;
  return SL2_OK;
}

extern "C" int sl2_frame_monitor_read(sl2_frame_monitor* m, int seq0, int nseq, sl2_frame_stats* stats, uint32_t* verdicts) {
  if (!m || !monitor_has_range(m, seq0, nseq)) { set_error("sl2_frame_monitor_read: bad arguments"); return SL2_ERR_INVALID; }
  SL2_HIP(hipSetDevice(m->device));
  if (m->queued) { SL2_HIP(hipEventSynchronize(m->done)); m->queued = false; }
  if (stats && nseq > 0) SL2_HIP(hipMemcpy(stats, m->d_stats + seq0, (size_t)nseq * sizeof(sl2_frame_stats), hipMemcpyDeviceToHost));
  if (verdicts && nseq > 0) SL2_HIP(hipMemcpy(verdicts, m->d_verdicts + seq0, (size_t)nseq * sizeof(uint32_t), hipMemcpyDeviceToHost));
  return SL2_OK;
}

extern "C" int sl2_frame_stats_host(const uint8_t* frame, int width, int height, sl2_frame_stats* stats) {
  if (!frame || !stats || !frame_size_ok(width, height)) {
    set_error("sl2_frame_stats_host: a frame, a record, width and height >= 1 and width * height < 2^31 are required");
    return SL2_ERR_INVALID;
  }
  frame_stats_host_body(frame, width, height, stats);
  return SL2_OK;
}

extern "C" uint32_t sl2_frame_verdict_host(const sl2_frame_stats* stats, const sl2_frame_gate* gate, int have_previous, uint64_t previous_digest) {
  if (!stats || !gate) { set_error("sl2_frame_verdict_host: bad arguments"); return 0xFFFFFFFFu; }
  if (const char* why = frame_gate_fault(*gate)) { set_error(std::string("sl2_frame_verdict_host: ") + why); return 0xFFFFFFFFu; }
  return frame_verdict(*stats, *gate, have_previous != 0, previous_digest);
}
