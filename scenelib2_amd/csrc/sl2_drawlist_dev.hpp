// Writing a draw list from a wavefront (DESIGN.md sections 8h-8j): what k_overlay_list, k_scene_list and k_world_list share.
// One wavefront lists one sequence.  Device code only - the SL2_HD headers beside it are also compiled into host programs.
#pragma once
#include "sl2_common.hpp"
#include "sl2_overlay_dev.hpp"

namespace sl2 {

constexpr int kListThreads = 256;
constexpr int kListSeqs = kListThreads / 64;      // sequences per workgroup of a list kernel, a wavefront each

__device__ __forceinline__ sl2_overlay_item draw_item(int kind, int label, int a0, int a1, int a2, int a3, const uint8_t rgb[3]) {
  sl2_overlay_item it = overlay_blank_item(kind, label);
  it.a[0] = a0; it.a[1] = a1; it.a[2] = a2; it.a[3] = a3;
  it.rgb[0] = rgb[0]; it.rgb[1] = rgb[1]; it.rgb[2] = rgb[2];
  return it;
}

// What a wavefront knows of the sequence it lists: list i of the call is sequence seq; o = its first feature slot, ns = its slots
// in use, xb = its state, psb = its partial slots' ps_i records, mark = the label to show as marked (-1: none).
struct SeqWave { int lane, i, seq, ns, mark; size_t o; const double* xb; const int* psb; };
__device__ __forceinline__ bool seq_wave(const SeqArrays& S, int seq0, int nseq, int N, int ld, int kpart, const int32_t* __restrict__ marked, SeqWave* q) {
  q->lane = threadIdx.x & 63;
  q->i = blockIdx.x * kListSeqs + (threadIdx.x >> 6);
  if (q->i >= nseq) return false;                      // (a whole wavefront)
  q->seq = seq0 + q->i;
  q->o = (size_t)q->seq * N;
  q->ns = min(max(S.n_slots[q->seq], 0), N);
  q->xb = S.x + (size_t)q->seq * ld;
  q->psb = S.ps_i + (size_t)q->seq * kpart * kPsInts;
  q->mark = marked ? marked[q->i] : -1;
  return true;
}

// The list of one sequence under the hands of its wavefront.  `total` is wave-uniform; one() and reserve() are called by all 64
// lanes together.  Nothing is stored at or beyond item_stride: every store goes through put().
struct ListWriter {
  sl2_overlay_item* list;
  int item_stride, total, lane;
  unsigned long long below;      // the lanes before this one

  __device__ __forceinline__ ListWriter(sl2_overlay_item* items, int i, int stride, int lane_)
      : list(items + (size_t)i * stride), item_stride(stride), total(0), lane(lane_), below((1ull << lane_) - 1ull) {}
  __device__ __forceinline__ void put(int at, const sl2_overlay_item& it) const {
    if (at < item_stride) list[at] = it;
  }
  // one item or none per lane, in lane order (a ballot): where this lane's goes
  __device__ __forceinline__ int one(bool ok) {
    const unsigned long long m = __ballot(ok);
    const int at = total + __popcll(m & below);
    total += __popcll(m);
    return at;
  }
  // c items per lane, in lane order (a shuffle scan): where this lane's first goes
  __device__ __forceinline__ int reserve(int c) {
    int incl = c;
    for (int d = 1; d < 64; d <<= 1) { const int t = __shfl_up(incl, d); if (lane >= d) incl += t; }
    const int at = total + incl - c;
    total += __shfl(incl, 63);
    return at;
  }
  __device__ __forceinline__ void finish(int32_t* counts, int i) const {
    if (lane == 0) counts[i] = total < item_stride ? total : item_stride;
  }
};

// what feature slot f of a sequence holds (o = the sequence's first slot, ns = its slots in use): nothing, a partially
// initialised feature's label, or a fully initialised feature
struct SlotClass { int fl, label; bool part, full; };
__device__ __forceinline__ SlotClass classify_slot(const SeqArrays& S, size_t o, int f, int ns) {
  SlotClass s;
  s.fl = f < ns ? S.f_flags[o + f] : 0;
  s.part = (s.fl & FF_PARTIAL) != 0;
  s.full = !s.part && (s.fl & FF_ACTIVE) != 0;
  s.label = (s.part || s.full) ? S.f_label[o + f] : -1;
  return s;
}

// the partial slot whose label sits in feature slot f (-1: none); psb = the sequence's ps_i records
__device__ __forceinline__ int partial_slot_of(const int* psb, int kpart, int f) {
  int ks = -1;
  for (int k = 0; k < kpart; ++k)
    if (psb[k * kPsInts + kPsActive] && psb[k * kPsInts + kPsLabel] == f) ks = k;
  return ks;
}

// The trajectory: a lane per pair of consecutive entries, 64 pairs a round, each a yellow segment or nothing.
// project(older end, newer end, c) -> whether the pair is seen, and its four coordinates.
template <class Project>
__device__ __forceinline__ void list_trajectory(ListWriter& w, const SeqArrays& S, int seq, Project project) {
  const int pushed = max(S.traj_count[seq], 0), have = min(pushed, kTrajCapacity), nseg = have - 1;
  const double* tr = S.traj + (size_t)seq * kTrajCapacity * 3;
  const uint8_t yellow[3] = {255, 255, 0};
  for (int base = 0; base < nseg; base += 64) {
    const int j = base + w.lane;
    bool ok = false;
    int c[4] = {0, 0, 0, 0};
    if (j < nseg) {
      const int first = pushed - have + j;          // the logical index of the older end: entry j of sl2_get_trajectory
      ok = project(tr + (size_t)(first % kTrajCapacity) * 3, tr + (size_t)((first + 1) % kTrajCapacity) * 3, c);
    }
    const int at = w.one(ok);
    if (ok) w.put(at, draw_item(SL2_ITEM_SEGMENT, -1, c[0], c[1], c[2], c[3], yellow));
  }
}

// What a lane found of its slot's feature, into the list in slot order: a marker (two RECTs), the ring of its uncertainty, the
// ray of a partial feature (a SEGMENT), in the colour of its state.  Called by all 64 lanes together.
__device__ __forceinline__ void list_feature(ListWriter& w, const SlotClass& s, int mark, bool has_marker, int mx, int my, bool has_ring, int rx, int ry,
                                             const double q[4], bool has_ray, const int ray[4]) {
  const int c = (has_marker ? 2 : 0) + (has_ring ? 1 : 0) + (has_ray ? 1 : 0);
  int at = w.reserve(c);
  if (c == 0) return;
  uint8_t rgb[3];
  overlay_colour(s.label == mark, s.full && (s.fl & FF_SELECTED) != 0, s.full && (s.fl & FF_SUCCESS) != 0, rgb);
  if (has_marker) {
    w.put(at, draw_item(SL2_ITEM_RECT, s.label, mx - 1, my - 1, mx + 1, my + 1, rgb));
    w.put(at + 1, draw_item(SL2_ITEM_RECT, s.label, mx, my, mx, my, rgb));
    at += 2;
  }
  if (has_ring) {
    sl2_overlay_item r = draw_item(SL2_ITEM_RING, s.label, rx, ry, 0, 0, rgb);
    r.q[0] = q[0]; r.q[1] = q[1]; r.q[2] = q[2]; r.q[3] = q[3];
    w.put(at, r);
  }
  if (has_ray) w.put(at, draw_item(SL2_ITEM_SEGMENT, s.label, ray[0], ray[1], ray[2], ray[3], rgb));
}

}  // namespace sl2
