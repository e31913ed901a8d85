// sl2_save_sequences / sl2_load_sequences / sl2_copy_sequences / sl2_reset_sequences (include/scenelib2_amd.h): the complete state
// of a sequence as a self-describing blob, written and read by the device.
//
// A sequence is ~30 arrays of the engine; at 100 features the dense covariance is > 95 % of its 0.8 MB.  k_seq_pack and
// k_seq_unpack are bandwidth kernels: the grid runs over (sequence, block of 16 rows of P) with the XCD-aware mapping of the
// update kernels, a wavefront moves whole rows in 16-byte pieces - engine rows at pitch ld, blob rows at the canonical pitch
// (13 + 3 n_slots + 6 partial slots, rounded up to 8 doubles) - and one more workgroup per sequence moves the small arrays and
// writes the header.  The partial features' columns sit at ppos = 13 + 3 N in an engine and right behind the slots in use in a
// blob: per row that is two segments with one index map each, not a map per element.  Unpacking writes EVERY row, column and
// slot of the destination (what the blob does not cover becomes zero: another sequence lived there a moment ago), so a reset is
// the unpack of an empty blob.
#include "sl2_common.hpp"
#include "sl2_mapmath.hpp"

namespace sl2 {

constexpr int kSlotArrays = SL2_BLOB_SLOT_ARRAYS;
constexpr int kSlotHcol = 8;           // the array whose values are state columns (f_hcol): re-based like the columns themselves
constexpr int kSeqBytes = 448;
constexpr int kCkptThreads = 256;
constexpr int kCkptRows = 16;          // rows of P per workgroup: four per wavefront
constexpr size_t kStageBytes = (size_t)64 << 20;   // staging of the host forms and of the copy: this much, or one blob if that is larger
static_assert(sizeof(sl2_sequence_blob_header) == 256, "sl2_sequence_blob_header is 256 bytes");
static_assert(kMaxPartial == 4 && kPartInts == 16 && kPsInts == 8 && kPsDoubles == 4 && kPartDoubles == 4, "layout of the blob's sequence section");
static_assert(kTrajCapacity * 24 % 64 == 0, "ring sections keep the 64-byte alignment");

// 4-byte words per slot of the blob's per-slot arrays, in blob order (the header comment of include/scenelib2_amd.h)
static const int kSlotWords[kSlotArrays] = {kPatchStride / 4, 2, 16, 1, 1, 1, 1, 1, 1, 4, 28, 12, 2, 8, 2, 4, 4, 1, 1, 2, 1, 1};

// What the two kernels take beside the engine's SeqArrays: the blob's per-slot arrays as a table they walk by index, and scalars.
struct CkptParams {
  unsigned* slot[kSlotArrays];
  int slot_words[kSlotArrays];
  int N, ld, ppos, kpart, pcap, mapping_used;
  int width, height;          // the engine's image size
  sl2_params prm;
};

__host__ __device__ inline unsigned up64(unsigned v) { return (v + 63u) & ~63u; }

// Offsets of the sections that follow the per-slot arrays (those are walked in order, each rounded up to 64 bytes).
struct BlobTail { unsigned off_seq, off_particles, off_traj, off_pos_log; unsigned long long bytes; };
__host__ __device__ inline void blob_front(int ns, int kp, unsigned* n, unsigned* pitch, unsigned* off_x, unsigned* off_P, unsigned* off_slots) {
  *n = 13u + 3u * (unsigned)ns + 6u * (unsigned)kp;
  *pitch = (*n + 7u) & ~7u;
  *off_x = 256u;
  *off_P = *off_x + *pitch * 8u;
  *off_slots = *off_P + *n * *pitch * 8u;      // (pitch * 8 is a multiple of 64)
}
__host__ __device__ inline BlobTail blob_tail(unsigned after_slots, int kp, int pc) {
  BlobTail t;
  t.off_seq = after_slots;
  t.off_particles = t.off_seq + kSeqBytes;
  t.off_traj = t.off_particles + up64((unsigned)kp * (unsigned)pc * kParticleDoubles * 8u);
  t.off_pos_log = t.off_traj + kTrajCapacity * 24u;
  t.bytes = (unsigned long long)t.off_pos_log + kTrajCapacity * 24u;
  return t;
}

// The whole layout on the host: offsets in the order sl2_sequence_blob_layout documents.
static size_t layout_host(int ns, int kp, int pc, uint64_t* out /* SL2_BLOB_LAYOUT_OFFSETS */, unsigned* n_out, unsigned* pitch_out) {
  unsigned n, pitch, ox, oP, os;
  blob_front(ns, kp, &n, &pitch, &ox, &oP, &os);
  out[0] = ox; out[1] = oP; out[2] = os;
  unsigned off = os;
  for (int a = 0; a < kSlotArrays; ++a) { out[3 + a] = off; off += up64((unsigned)ns * kSlotWords[a] * 4u); }
  const BlobTail t = blob_tail(off, kp, pc);
  out[3 + kSlotArrays] = t.off_seq; out[4 + kSlotArrays] = t.off_particles; out[5 + kSlotArrays] = t.off_traj; out[6 + kSlotArrays] = t.off_pos_log;
  if (n_out) *n_out = n;
  if (pitch_out) *pitch_out = pitch;
  return (size_t)t.bytes;
}

// ----------------------------------------------------------------------------------------------------------------- pack
// tiles - 1 row blocks of P, then the workgroup of the small arrays (header_only: that one alone, and of it the header alone:
// what sl2_copy_sequences checks before it writes anything).
__global__ void __launch_bounds__(kCkptThreads) k_seq_pack(const SeqArrays S, const CkptParams A, int seq0, int nseq, int tiles,
                                                           unsigned char* __restrict__ blobs, size_t stride, int header_only) {
  int s, tile;
  if (!xcd_map(tiles, nseq, &s, &tile)) return;
  const int b = seq0 + s, tid = threadIdx.x;
  unsigned char* blob = blobs + (size_t)s * stride;
  int ns = S.n_slots[b];
  ns = ns < 0 ? 0 : (ns > A.N ? A.N : ns);
  int kp = 0, pc = 0;
  for (int k = 0; k < A.kpart; ++k) {
    const int* ps = S.ps_i + ((size_t)b * A.kpart + k) * kPsInts;
    if (ps[kPsActive]) { kp = k + 1; const int np = ps[kPsNp]; pc = np > pc ? np : pc; }
  }
  pc = pc < 0 ? 0 : (pc > A.pcap ? A.pcap : pc);
  unsigned n, pitch, off_x, off_P, off_slots;
  blob_front(ns, kp, &n, &pitch, &off_x, &off_P, &off_slots);
  const int c1 = 13 + 3 * ns, ppos = A.ppos;
  if (tile < tiles - 1) {
    const int lane = tid & 63, wave = tid >> 6;
    const int r_end = (tile + 1) * kCkptRows < (int)n ? (tile + 1) * kCkptRows : (int)n;
    for (int r = tile * kCkptRows + wave; r < r_end; r += kCkptThreads / 64) {
      const int re = r < c1 ? r : ppos + (r - c1);
      const double* __restrict__ src = S.P + (size_t)b * A.ld * A.ld + (size_t)re * A.ld;
      double* __restrict__ dst = reinterpret_cast<double*>(blob + off_P) + (size_t)r * pitch;
      for (int c = 2 * lane; c < (int)pitch; c += 128) {
        double2 v;
        if (c + 1 < c1) v = *reinterpret_cast<const double2*>(src + c);          // the slots' segment: same columns on both sides
        else {
          v.x = c < c1 ? src[c] : (c < (int)n ? src[ppos + (c - c1)] : 0.0);
          v.y = c + 1 < c1 ? src[c + 1] : (c + 1 < (int)n ? src[ppos + (c + 1 - c1)] : 0.0);
        }
        *reinterpret_cast<double2*>(dst + c) = v;
      }
    }
    return;
  }
  // ---- the small arrays
  unsigned off = off_slots;
  for (int a = 0; a < kSlotArrays; ++a) off += up64((unsigned)ns * A.slot_words[a] * 4u);
  const BlobTail t = blob_tail(off, kp, pc);
  if (!header_only) {
    const double* xb = S.x + (size_t)b * A.ld;
    double* ox = reinterpret_cast<double*>(blob + off_x);
    for (int c = tid; c < (int)pitch; c += kCkptThreads) ox[c] = c < c1 ? xb[c] : (c < (int)n ? xb[ppos + (c - c1)] : 0.0);
    off = off_slots;
    for (int a = 0; a < kSlotArrays; ++a) {
      const int w = A.slot_words[a], tot = ns * w, padded = (tot + 15) & ~15;
      const unsigned* __restrict__ src = A.slot[a] + (size_t)b * A.N * w;
      unsigned* __restrict__ dst = reinterpret_cast<unsigned*>(blob + off);
      for (int i = tid; i < padded; i += kCkptThreads) {
        unsigned v = i < tot ? src[i] : 0u;
        if (a == kSlotHcol && i < tot && (int)v >= ppos) v = v - ppos + c1;
        dst[i] = v;
      }
      off += padded * 4u;
    }
    __shared__ double s_seq[kSeqBytes / 8];
    for (int i = tid; i < kSeqBytes / 8; i += kCkptThreads) s_seq[i] = 0.0;
    __syncthreads();
    int* qi = reinterpret_cast<int*>(s_seq);
    if (tid == 0) {
      qi[0] = ns; qi[1] = S.next_label[b]; qi[2] = S.status[b]; qi[3] = S.pos_err_any[b]; qi[4] = S.n_sel[b]; qi[5] = S.n_vis[b];
      qi[6] = S.m_count[b]; qi[7] = S.traj_count[b];
      *reinterpret_cast<unsigned long long*>(s_seq + 4) = S.rand48[b];
      for (int k = 0; k < 3; ++k) { s_seq[5 + k] = S.prev_r[b * 3 + k]; s_seq[8 + k] = S.last_r[b * 3 + k]; }
      for (int k = 0; k < kPartDoubles; ++k) s_seq[11 + k] = S.part_d[(size_t)b * kPartDoubles + k];
    }
    if (tid < kPartInts) qi[32 + tid] = S.part_i[(size_t)b * kPartInts + tid];
    if (tid >= 64 && tid < 64 + kp * kPsInts) qi[48 + tid - 64] = S.ps_i[(size_t)b * A.kpart * kPsInts + tid - 64];
    if (tid >= 128 && tid < 128 + kp * kPsDoubles) s_seq[40 + tid - 128] = S.ps_d[(size_t)b * A.kpart * kPsDoubles + tid - 128];
    __syncthreads();
    double* oq = reinterpret_cast<double*>(blob + t.off_seq);
    for (int i = tid; i < kSeqBytes / 8; i += kCkptThreads) oq[i] = s_seq[i];
    double* op = reinterpret_cast<double*>(blob + t.off_particles);
    const int per = pc * kParticleDoubles, ptot = kp * per, ppad = (ptot + 7) & ~7;
    for (int i = tid; i < ppad; i += kCkptThreads)
      op[i] = i < ptot ? S.particles[((size_t)b * A.kpart + i / per) * A.pcap * kParticleDoubles + i % per] : 0.0;
    double* ot = reinterpret_cast<double*>(blob + t.off_traj);
    const double* tr = S.traj + (size_t)b * kTrajCapacity * 3;
    for (int i = tid; i < kTrajCapacity * 3; i += kCkptThreads) ot[i] = tr[i];
    double* ol = reinterpret_cast<double*>(blob + t.off_pos_log);
    const double* lg = S.pos_log + (size_t)b * kTrajCapacity * 3;
    // oldest first, the newest entry last.  The ring is indexed by the ENGINE's step; how far back it holds this sequence is
    // the sequence's own age (a loaded sequence brought entries from before this engine's first step along).
    const int steps = S.pos_count[b];
    const long long own = (long long)steps + S.seq_age[b];
    for (int i = tid; i < kTrajCapacity * 3; i += kCkptThreads) {
      const int j = i / 3;
      int slot = (steps - kTrajCapacity + j) % kTrajCapacity;
      if (slot < 0) slot += kTrajCapacity;
      ol[i] = (long long)(kTrajCapacity - j) <= own ? lg[slot * 3 + i % 3] : 0.0;
    }
  }
  // the header goes last: whoever finds it behind this workgroup's stores finds the small sections complete (the rows of P are
  // other workgroups' work and complete when the launch is)
  __shared__ sl2_sequence_blob_header hd;
  if (tid < 64) reinterpret_cast<int*>(&hd)[tid] = 0;
  __threadfence();
  __syncthreads();
  if (tid == 0) {
    hd.magic = SL2_BLOB_MAGIC; hd.layout_version = SL2_BLOB_LAYOUT_VERSION; hd.bytes = t.bytes;
    hd.sequence_steps = (long long)S.pos_count[b] + S.seq_age[b];
    hd.src_max_features = A.N; hd.src_partial_slots = A.kpart; hd.src_particle_capacity = A.pcap;
    hd.width = A.width; hd.height = A.height;
    hd.n_slots = ns; hd.n_partial_slots = kp; hd.n_particles = pc; hd.mapping_in_use = A.mapping_used;
    hd.off_x = off_x; hd.off_P = off_P; hd.off_slots = off_slots; hd.off_seq = t.off_seq; hd.off_particles = t.off_particles;
    hd.off_traj = t.off_traj; hd.off_pos_log = t.off_pos_log;
    hd.row_pitch = (int)pitch; hd.state_size = (int)n;
    {   // the calibration the sequence ran under: its own record (the sl2_create camera's values until sl2_set_cameras)
      const double* rec = S.seq_cam + (size_t)b * kSeqCamDoubles;
      hd.camera.width = A.width; hd.camera.height = A.height;
      hd.camera.fku = rec[kSeqCamFku]; hd.camera.fkv = rec[kSeqCamFkv]; hd.camera.u0 = rec[kSeqCamU0]; hd.camera.v0 = rec[kSeqCamV0];
      hd.camera.kd1 = rec[kSeqCamKd1]; hd.camera.sd = (int)rec[kSeqCamSd];
    }
    hd.params = A.prm;
    hd.n_selected = S.n_sel[b];
  }
  __syncthreads();
  if (tid < 64) reinterpret_cast<int*>(blob)[tid] = reinterpret_cast<const int*>(&hd)[tid];
}

// --------------------------------------------------------------------------------------------------------------- unpack
// blobs == nullptr: the empty blob (sl2_reset_sequences).  Headers were checked on the host; a blob that does not fit is left
// alone here all the same (nothing is written outside the destination's arrays whatever the bytes say).
__global__ void __launch_bounds__(kCkptThreads) k_seq_unpack(const SeqArrays S, const CkptParams A, int seq0, int nseq, int tiles,
                                                             const unsigned char* __restrict__ blobs, size_t stride, long long steps_done) {
  int s, tile;
  if (!xcd_map(tiles, nseq, &s, &tile)) return;
  const int b = seq0 + s, tid = threadIdx.x;
  const unsigned char* blob = blobs ? blobs + (size_t)s * stride : nullptr;
  int ns = 0, kp = 0, pc = 0;
  long long age = 0;
  if (blob) {
    const sl2_sequence_blob_header* h = reinterpret_cast<const sl2_sequence_blob_header*>(blob);
    ns = h->n_slots; kp = h->n_partial_slots; pc = h->n_particles; age = h->sequence_steps;
    if (h->magic != SL2_BLOB_MAGIC || ns < 0 || ns > A.N || kp < 0 || kp > A.kpart || pc < 0 || pc > A.pcap) return;
  }
  unsigned n, pitch, off_x, off_P, off_slots;
  blob_front(ns, kp, &n, &pitch, &off_x, &off_P, &off_slots);
  const int c1 = 13 + 3 * ns, ppos = A.ppos, pend = ppos + 6 * kp, ld = A.ld;
  if (tile < tiles - 1) {
    const int lane = tid & 63, wave = tid >> 6;
    const int r_end = (tile + 1) * kCkptRows < ld ? (tile + 1) * kCkptRows : ld;
    for (int r = tile * kCkptRows + wave; r < r_end; r += kCkptThreads / 64) {
      const int rb = !blob ? -1 : (r < c1 ? r : (r >= ppos && r < pend ? c1 + (r - ppos) : -1));
      double* __restrict__ dst = S.P + (size_t)b * ld * ld + (size_t)r * ld;
      const double* __restrict__ src = rb >= 0 ? reinterpret_cast<const double*>(blob + off_P) + (size_t)rb * pitch : nullptr;
      for (int c = 2 * lane; c < ld; c += 128) {
        double2 v = make_double2(0.0, 0.0);
        if (src) {
          if (c + 1 < c1) v = *reinterpret_cast<const double2*>(src + c);
          else {
            v.x = c < c1 ? src[c] : (c >= ppos && c < pend ? src[c1 + (c - ppos)] : 0.0);
            v.y = c + 1 < c1 ? src[c + 1] : (c + 1 >= ppos && c + 1 < pend ? src[c1 + (c + 1 - ppos)] : 0.0);
          }
        }
        *reinterpret_cast<double2*>(dst + c) = v;
      }
    }
    return;
  }
  // ---- the small arrays
  {
    double* xb = S.x + (size_t)b * ld;
    const double* ix = blob ? reinterpret_cast<const double*>(blob + off_x) : nullptr;
    for (int c = tid; c < ld; c += kCkptThreads) xb[c] = !ix ? 0.0 : (c < c1 ? ix[c] : (c >= ppos && c < pend ? ix[c1 + (c - ppos)] : 0.0));
  }
  unsigned off = off_slots;
  for (int a = 0; a < kSlotArrays; ++a) {
    const int w = A.slot_words[a], tot = ns * w, all = A.N * w;
    unsigned* __restrict__ dst = A.slot[a] + (size_t)b * A.N * w;
    const unsigned* __restrict__ src = blob ? reinterpret_cast<const unsigned*>(blob + off) : nullptr;
    for (int i = tid; i < all; i += kCkptThreads) {
      unsigned v = i < tot ? src[i] : 0u;
      if (a == kSlotHcol && i < tot && (int)v >= c1) v = v - c1 + ppos;
      dst[i] = v;
    }
    off += up64((unsigned)tot * 4u);
  }
  const BlobTail t = blob_tail(off, kp, pc);
  __shared__ double s_seq[kSeqBytes / 8];
  const double* iq = blob ? reinterpret_cast<const double*>(blob + t.off_seq) : nullptr;
  for (int i = tid; i < kSeqBytes / 8; i += kCkptThreads) s_seq[i] = iq ? iq[i] : 0.0;
  __syncthreads();
  const int* qi = reinterpret_cast<const int*>(s_seq);
  if (tid == 0) {
    S.n_slots[b] = ns; S.next_label[b] = qi[1]; S.status[b] = qi[2]; S.pos_err_any[b] = qi[3]; S.n_sel[b] = qi[4]; S.n_vis[b] = qi[5];
    S.m_count[b] = qi[6]; S.traj_count[b] = qi[7];
    S.sel_gate[b] = qi[4]; S.m_gate[b] = qi[6];       // the per-step gates (sl2_common.hpp) follow what they gate: a seam called next finds the loaded frame
    S.step_mark[b] = 0;                               // ... but the record of sl2_get_step_stats starts again: this sequence has not stepped HERE
    S.rand48[b] = blob ? *reinterpret_cast<const unsigned long long*>(s_seq + 4) : kRand48Seed0;
    for (int k = 0; k < 3; ++k) { S.prev_r[b * 3 + k] = s_seq[5 + k]; S.last_r[b * 3 + k] = s_seq[8 + k]; }
    for (int k = 0; k < kPartDoubles; ++k) S.part_d[(size_t)b * kPartDoubles + k] = s_seq[11 + k];
    // the step clock is the destination's (finalize_body and k_map_update publish pos_count, the host compares it with steps_done)
    S.pos_count[b] = (int)steps_done;
    S.seq_age[b] = (int)(age - steps_done);
  }
  if (tid < kPartInts) S.part_i[(size_t)b * kPartInts + tid] = qi[32 + tid];
  if (tid >= 64 && tid < 64 + A.kpart * kPsInts) S.ps_i[(size_t)b * A.kpart * kPsInts + tid - 64] = tid - 64 < kp * kPsInts ? qi[48 + tid - 64] : 0;
  if (tid >= 128 && tid < 128 + A.kpart * kPsDoubles) S.ps_d[(size_t)b * A.kpart * kPsDoubles + tid - 128] = tid - 128 < kp * kPsDoubles ? s_seq[40 + tid - 128] : 0.0;
  {
    const double* ip = blob ? reinterpret_cast<const double*>(blob + t.off_particles) : nullptr;
    const int per = pc * kParticleDoubles, cap = A.pcap * kParticleDoubles;
    double* dp = S.particles + (size_t)b * A.kpart * cap;
    for (int i = tid; i < A.kpart * cap; i += kCkptThreads) {
      const int k = i / cap, j = i % cap;
      dp[i] = (k < kp && j < per) ? ip[k * per + j] : 0.0;
    }
  }
  {
    const double* it = blob ? reinterpret_cast<const double*>(blob + t.off_traj) : nullptr;
    double* tr = S.traj + (size_t)b * kTrajCapacity * 3;
    for (int i = tid; i < kTrajCapacity * 3; i += kCkptThreads) tr[i] = it ? it[i] : 0.0;
    const double* il = blob ? reinterpret_cast<const double*>(blob + t.off_pos_log) : nullptr;
    double* lg = S.pos_log + (size_t)b * kTrajCapacity * 3;
    for (int i = tid; i < kTrajCapacity * 3; i += kCkptThreads) {
      long long logical = (steps_done - kTrajCapacity + i / 3) % kTrajCapacity;     // the blob's newest entry becomes the destination's newest
      if (logical < 0) logical += kTrajCapacity;
      lg[logical * 3 + i % 3] = il ? il[i] : 0.0;
    }
  }
}

// ----------------------------------------------------------------------------------------------------------------- host

static CkptParams ckpt_params(sl2_engine* e) {
  CkptParams A;
  memset(&A, 0, sizeof(A));
  void* slot[kSlotArrays] = {e->patch, e->patch_sums, e->xp_org, e->f_flags, e->f_label, e->attempted, e->successful, e->pos_err, e->f_hcol,
                             e->f_h, e->f_Hx, e->f_Hy, e->f_R, e->f_S, e->f_score, e->f_z, e->f_nu, e->sel_idx, e->meas_ok, e->meas_score,
                             e->succ_idx, e->f_arow};
  for (int a = 0; a < kSlotArrays; ++a) { A.slot[a] = (unsigned*)slot[a]; A.slot_words[a] = kSlotWords[a]; }
  A.N = e->N; A.ld = e->ld; A.ppos = e->ppos; A.kpart = e->kpart; A.pcap = e->pcap; A.mapping_used = e->mapping_used ? 1 : 0;
  // (field by field into zeroed structures: the blob's copies carry no padding bytes of the caller's)
  A.width = e->cam.width; A.height = e->cam.height;
  const sl2_params& p = e->prm;
  A.prm.delta_t = p.delta_t; A.prm.number_of_features_to_select = p.number_of_features_to_select;
  A.prm.number_of_features_to_keep_visible = p.number_of_features_to_keep_visible;
  A.prm.max_features_to_init_at_once = p.max_features_to_init_at_once; A.prm.min_lambda = p.min_lambda; A.prm.max_lambda = p.max_lambda;
  A.prm.number_of_particles = p.number_of_particles; A.prm.standard_deviation_depth_ratio = p.standard_deviation_depth_ratio;
  A.prm.min_number_of_particles = p.min_number_of_particles; A.prm.prune_probability_threshold = p.prune_probability_threshold;
  A.prm.erase_partially_init_feature_after_this_many_attempts = p.erase_partially_init_feature_after_this_many_attempts;
  A.prm.minimum_attempted_measurements_of_feature = p.minimum_attempted_measurements_of_feature;
  A.prm.successful_match_fraction = p.successful_match_fraction;
  return A;
}

static int pack_tiles(const sl2_engine* e) { return (13 + 3 * e->N + 6 * e->kpart + kCkptRows - 1) / kCkptRows + 1; }
static int unpack_tiles(const sl2_engine* e) { return (e->ld + kCkptRows - 1) / kCkptRows + 1; }

static int launch_pack(sl2_engine* e, int seq0, int nseq, void* blobs, size_t stride, int header_only, hipStream_t st) {
  const int tiles = header_only ? 1 : pack_tiles(e);
  LaunchScope ls(e, "k_seq_pack");
  hipLaunchKernelGGL(k_seq_pack, dim3(xcd_grid(tiles, nseq)), dim3(kCkptThreads), 0, st, seq_arrays(e), ckpt_params(e), seq0, nseq, tiles,
                     (unsigned char*)blobs, stride, header_only);
  SL2_HIP(hipGetLastError());
  return SL2_OK;
}
static int launch_unpack(sl2_engine* e, int seq0, int nseq, const void* blobs, size_t stride, hipStream_t st) {
  const int tiles = unpack_tiles(e);
  LaunchScope ls(e, "k_seq_unpack");
  hipLaunchKernelGGL(k_seq_unpack, dim3(xcd_grid(tiles, nseq)), dim3(kCkptThreads), 0, st, seq_arrays(e), ckpt_params(e), seq0, nseq, tiles,
                     (const unsigned char*)blobs, stride, e->steps_done);
  SL2_HIP(hipGetLastError());
  return SL2_OK;
}

static size_t capacity_of(const sl2_engine* e) {
  uint64_t off[SL2_BLOB_LAYOUT_OFFSETS];
  return layout_host(e->N, e->kpart, e->pcap, off, nullptr, nullptr);
}

// Engine-owned staging: grown on demand (after a synchronisation: hipFree waits for the device anyway), never beyond what a
// chunk needs.
static int stage_for(sl2_engine* e, size_t bytes) {
  if (bytes <= e->ckpt_stage_bytes) return SL2_OK;
  { int rc = e->sync_all(); if (rc != SL2_OK) return rc; }
  if (e->ckpt_stage) { SL2_HIP(hipFree(e->ckpt_stage)); e->ckpt_stage = nullptr; e->ckpt_stage_bytes = 0; }
  SL2_HIP(hipMalloc(&e->ckpt_stage, bytes));
  SL2_HIP(hipMemset(e->ckpt_stage, 0, bytes));
  e->ckpt_stage_bytes = bytes;
  return SL2_OK;
}
static int chunk_of(size_t cap, int nseq) {
  size_t c = kStageBytes / cap;
  if (c < 1) c = 1;
  return c < (size_t)nseq ? (int)c : nseq;
}

void release_checkpoint_staging(sl2_engine* e) {
  if (e->ckpt_stage) hipFree(e->ckpt_stage);
  if (e->ckpt_event) hipEventDestroy(e->ckpt_event);
  e->ckpt_stage = nullptr; e->ckpt_stage_bytes = 0; e->ckpt_event = nullptr;
}

static int refuse(int code, int index, const char* field, const char* what) {
  char buf[256];
  snprintf(buf, sizeof(buf), "sequence blob %d: %s: %s", index, field, what);
  set_error(buf);
  return code;
}

// Does blob `index` (its header; `avail` bytes of it exist) describe a well-formed blob that fits sequence dst_seq of engine e?
// (The calibration is the destination SEQUENCE's, from the host's mirror of seq_cam: a map continued under another camera is
// silently wrong, so the caller gives the slot the sequence's camera - sl2_set_cameras - before it loads or copies into it.)
// (engine_to_engine: sl2_copy_sequences.  The time step is the destination's own record and travels in no blob, so two
// engines created with different params.delta_t - cameras of different rates - may still hand sequences to each other; a blob
// from outside is held to every word of params as before.)
static int check_header(sl2_engine* e, int dst_seq, const sl2_sequence_blob_header& h, size_t avail, int index, bool engine_to_engine = false) {
  if (h.magic != SL2_BLOB_MAGIC) return refuse(SL2_ERR_INVALID, index, "magic", "not a sequence blob");
  if (h.layout_version != SL2_BLOB_LAYOUT_VERSION) return refuse(SL2_ERR_INVALID, index, "layout_version", "unknown layout");
  if (h.n_slots < 0 || h.n_slots > 676) return refuse(SL2_ERR_INVALID, index, "n_slots", "out of range");
  if (h.n_partial_slots < 0 || h.n_partial_slots > kMaxPartial) return refuse(SL2_ERR_INVALID, index, "n_partial_slots", "out of range");
  if (h.n_particles < 0 || h.n_particles > kMaxParticles) return refuse(SL2_ERR_INVALID, index, "n_particles", "out of range");
  uint64_t off[SL2_BLOB_LAYOUT_OFFSETS];
  unsigned n, pitch;
  const size_t bytes = layout_host(h.n_slots, h.n_partial_slots, h.n_particles, off, &n, &pitch);
  if (h.bytes != bytes) return refuse(SL2_ERR_INVALID, index, "bytes", "does not match the sizes in the header");
  if (h.bytes > avail) return refuse(SL2_ERR_INVALID, index, "bytes", "the blob is truncated (larger than the bytes given)");
  if (h.off_x != off[0] || h.off_P != off[1] || h.off_slots != off[2] || h.off_seq != off[3 + kSlotArrays] ||
      h.off_particles != off[4 + kSlotArrays] || h.off_traj != off[5 + kSlotArrays] || h.off_pos_log != off[6 + kSlotArrays] ||
      h.row_pitch != (int)pitch || h.state_size != (int)n)
    return refuse(SL2_ERR_INVALID, index, "section offsets", "do not match the layout");
  const CkptParams A = ckpt_params(e);
  if (memcmp(&h.camera, &e->cams_host[dst_seq], sizeof(sl2_camera)) != 0 || h.width != A.width || h.height != A.height)
    return refuse(SL2_ERR_INVALID, index, "camera", "differs from the destination sequence's");
  sl2_params p = h.params;
  p.max_features_to_init_at_once = A.prm.max_features_to_init_at_once;
  p.number_of_features_to_select = A.prm.number_of_features_to_select;
  if (engine_to_engine) p.delta_t = A.prm.delta_t;
  if (memcmp(&p, &A.prm, sizeof(sl2_params)) != 0) return refuse(SL2_ERR_INVALID, index, "params", "differ from the engine's");
  if (h.n_slots > e->N) return refuse(SL2_ERR_CAPACITY, index, "n_slots", "more feature slots than the engine's max_features");
  if (h.n_partial_slots > e->kpart) return refuse(SL2_ERR_CAPACITY, index, "n_partial_slots", "more partial slots than the engine's max_features_to_init_at_once");
  if (h.n_particles > e->pcap) return refuse(SL2_ERR_CAPACITY, index, "n_particles", "more particles than the engine's particle capacity");
  if (h.n_selected < 0 || h.n_selected > e->nsel_max) return refuse(SL2_ERR_CAPACITY, index, "n_selected", "more selected features than the engine's number_of_features_to_select");
  if (h.mapping_in_use && !e->mapping_used && e->groups.size() > 1)
    return refuse(SL2_ERR_INVALID, index, "mapping_in_use", "feature initialisation is not available with sequence groups (sl2_set_groups > 1)");
  return SL2_OK;
}

// Before the first unpack of a call: the device is idle, no captured step survives, feature initialisation is on if a blob needs it.
static int prepare_destination(sl2_engine* e, bool mapping) {
  { int rc = e->sync_all(); if (rc != SL2_OK) return rc; }
  { int rc = checkpoint_drop_graphs(e); if (rc != SL2_OK) return rc; }
  if (mapping && !e->mapping_used) { int rc = checkpoint_enable_mapping(e); if (rc != SL2_OK) return rc; }
  return SL2_OK;
}
// After the last one: the exact map sizes, and the next step does not trust the partial-feature mailbox.
static int settle_destination(sl2_engine* e) {
  { int rc = e->sync_all(); if (rc != SL2_OK) return rc; }
  e->parts_block_step = e->steps_done;
  return checkpoint_refresh_slots(e);
}

static bool range_ok(const sl2_engine* e, int seq0, int nseq) { return e && seq0 >= 0 && nseq > 0 && seq0 <= e->B - nseq; }

}  // namespace sl2

using namespace sl2;

extern "C" {

size_t sl2_sequence_blob_layout(int n_slots, int n_partial_slots, int n_particles, uint64_t* offsets, int capacity) {
  if (n_slots < 0 || n_partial_slots < 0 || n_particles < 0 || n_slots > 676 || n_partial_slots > kMaxPartial || n_particles > kMaxParticles) return 0;
  uint64_t off[SL2_BLOB_LAYOUT_OFFSETS];
  const size_t bytes = layout_host(n_slots, n_partial_slots, n_particles, off, nullptr, nullptr);
  for (int k = 0; offsets && k < capacity && k < SL2_BLOB_LAYOUT_OFFSETS; ++k) offsets[k] = off[k];
  return bytes;
}

size_t sl2_sequence_blob_capacity(const sl2_engine* e) { return e ? capacity_of(e) : 0; }

int sl2_save_sequences(sl2_engine* e, int seq0, int nseq, void* blobs, size_t blob_stride, int blobs_on_device, uint64_t* bytes) {
  if (!range_ok(e, seq0, nseq) || !blobs) { set_error("sl2_save_sequences: bad argument"); return SL2_ERR_INVALID; }
  const size_t cap = capacity_of(e);
  if (blob_stride < cap || blob_stride % 64) { set_error("sl2_save_sequences: blob_stride must be a multiple of 64 and at least sl2_sequence_blob_capacity"); return SL2_ERR_INVALID; }
  if (blobs_on_device && (uintptr_t)blobs % 64) { set_error("sl2_save_sequences: device blobs must start on a 64-byte boundary"); return SL2_ERR_INVALID; }
  if (blobs_on_device && bytes) { set_error("sl2_save_sequences: bytes must be NULL for device blobs (the size is in each header)"); return SL2_ERR_INVALID; }
  SL2_HIP(hipSetDevice(e->device));
  if (blobs_on_device) return launch_pack(e, seq0, nseq, blobs, blob_stride, 0, e->stream);
  const int chunk = chunk_of(cap, nseq);
  { int rc = stage_for(e, (size_t)chunk * cap); if (rc != SL2_OK) return rc; }
  for (int c0 = 0; c0 < nseq; c0 += chunk) {
    const int m = nseq - c0 < chunk ? nseq - c0 : chunk;
    { int rc = launch_pack(e, seq0 + c0, m, e->ckpt_stage, cap, 0, e->stream); if (rc != SL2_OK) return rc; }
    SL2_HIP(hipMemcpy2DAsync((char*)blobs + (size_t)c0 * blob_stride, blob_stride, e->ckpt_stage, cap, cap, m, hipMemcpyDeviceToHost, e->stream));
    SL2_HIP(hipStreamSynchronize(e->stream));
    for (int i = 0; bytes && i < m; ++i) bytes[c0 + i] = ((const sl2_sequence_blob_header*)((const char*)blobs + (size_t)(c0 + i) * blob_stride))->bytes;
  }
  return SL2_OK;
}

int sl2_load_sequences(sl2_engine* e, int seq0, int nseq, const void* blobs, size_t blob_stride, int blobs_on_device) {
  if (!range_ok(e, seq0, nseq) || !blobs) { set_error("sl2_load_sequences: bad argument"); return SL2_ERR_INVALID; }
  if (blob_stride < sizeof(sl2_sequence_blob_header) || blob_stride % 64) { set_error("sl2_load_sequences: blob_stride must be a multiple of 64 that holds a blob"); return SL2_ERR_INVALID; }
  if (blobs_on_device && (uintptr_t)blobs % 64) { set_error("sl2_load_sequences: device blobs must start on a 64-byte boundary"); return SL2_ERR_INVALID; }
  SL2_HIP(hipSetDevice(e->device));
  std::vector<sl2_sequence_blob_header> hs(nseq);
  if (blobs_on_device) {
    SL2_HIP(hipMemcpy2DAsync(hs.data(), sizeof(sl2_sequence_blob_header), blobs, blob_stride, sizeof(sl2_sequence_blob_header), nseq, hipMemcpyDeviceToHost, e->stream));
    SL2_HIP(hipStreamSynchronize(e->stream));
  } else {
    for (int i = 0; i < nseq; ++i) memcpy(&hs[i], (const char*)blobs + (size_t)i * blob_stride, sizeof(sl2_sequence_blob_header));
  }
  bool mapping = false;
  size_t largest = 0;
  for (int i = 0; i < nseq; ++i) {
    const int rc = check_header(e, seq0 + i, hs[i], blob_stride, i);
    if (rc != SL2_OK) return rc;
    mapping = mapping || hs[i].mapping_in_use != 0;
    largest = hs[i].bytes > largest ? (size_t)hs[i].bytes : largest;
  }
  { int rc = prepare_destination(e, mapping); if (rc != SL2_OK) return rc; }
  if (blobs_on_device) {
    int rc = launch_unpack(e, seq0, nseq, blobs, blob_stride, e->stream);
    if (rc != SL2_OK) return rc;
  } else {
    const int chunk = chunk_of(largest, nseq);
    { int rc = stage_for(e, (size_t)chunk * largest); if (rc != SL2_OK) return rc; }
    for (int c0 = 0; c0 < nseq; c0 += chunk) {
      const int m = nseq - c0 < chunk ? nseq - c0 : chunk;
      for (int i = 0; i < m; ++i)
        SL2_HIP(hipMemcpyAsync((char*)e->ckpt_stage + (size_t)i * largest, (const char*)blobs + (size_t)(c0 + i) * blob_stride, (size_t)hs[c0 + i].bytes,
                               hipMemcpyHostToDevice, e->stream));
      { int rc = launch_unpack(e, seq0 + c0, m, e->ckpt_stage, largest, e->stream); if (rc != SL2_OK) return rc; }
      SL2_HIP(hipStreamSynchronize(e->stream));
    }
  }
  return settle_destination(e);
}

int sl2_copy_sequences(sl2_engine* dst, int dst_seq0, sl2_engine* src, int src_seq0, int nseq) {
  if (!range_ok(dst, dst_seq0, nseq) || !range_ok(src, src_seq0, nseq)) { set_error("sl2_copy_sequences: bad argument"); return SL2_ERR_INVALID; }
  if (dst->device != src->device) { set_error("sl2_copy_sequences: the engines are on different devices"); return SL2_ERR_INVALID; }
  if (dst == src && dst_seq0 < src_seq0 + nseq && src_seq0 < dst_seq0 + nseq) { set_error("sl2_copy_sequences: the ranges overlap"); return SL2_ERR_INVALID; }
  SL2_HIP(hipSetDevice(src->device));
  const size_t cap = capacity_of(src);
  const int chunk = chunk_of(cap, nseq);
  { int rc = stage_for(src, (size_t)chunk * cap); if (rc != SL2_OK) return rc; }
  // the headers alone first: every one is checked against the destination before anything is written
  std::vector<sl2_sequence_blob_header> hs(nseq);
  bool mapping = false;
  for (int c0 = 0; c0 < nseq; c0 += chunk) {
    const int m = nseq - c0 < chunk ? nseq - c0 : chunk;
    { int rc = launch_pack(src, src_seq0 + c0, m, src->ckpt_stage, cap, 1, src->stream); if (rc != SL2_OK) return rc; }
    SL2_HIP(hipMemcpy2DAsync(&hs[c0], sizeof(sl2_sequence_blob_header), src->ckpt_stage, cap, sizeof(sl2_sequence_blob_header), m, hipMemcpyDeviceToHost, src->stream));
    SL2_HIP(hipStreamSynchronize(src->stream));
  }
  for (int i = 0; i < nseq; ++i) {
    const int rc = check_header(dst, dst_seq0 + i, hs[i], cap, i, true);
    if (rc != SL2_OK) return rc;
    mapping = mapping || hs[i].mapping_in_use != 0;
  }
  { int rc = prepare_destination(dst, mapping); if (rc != SL2_OK) return rc; }
  if (!src->ckpt_event) SL2_HIP(hipEventCreateWithFlags(&src->ckpt_event, hipEventDisableTiming));
  for (int c0 = 0; c0 < nseq; c0 += chunk) {
    const int m = nseq - c0 < chunk ? nseq - c0 : chunk;
    { int rc = launch_pack(src, src_seq0 + c0, m, src->ckpt_stage, cap, 0, src->stream); if (rc != SL2_OK) return rc; }
    if (dst->stream != src->stream) {       // the unpack waits for the pack: an event, not a device-wide synchronisation
      SL2_HIP(hipEventRecord(src->ckpt_event, src->stream));
      SL2_HIP(hipStreamWaitEvent(dst->stream, src->ckpt_event, 0));
    }
    { int rc = launch_unpack(dst, dst_seq0 + c0, m, src->ckpt_stage, cap, dst->stream); if (rc != SL2_OK) return rc; }
    SL2_HIP(hipStreamSynchronize(dst->stream));     // (the staging is the next chunk's, too)
  }
  return settle_destination(dst);
}

int sl2_reset_sequences(sl2_engine* e, int seq0, int nseq) {
  if (!range_ok(e, seq0, nseq)) { set_error("sl2_reset_sequences: bad argument"); return SL2_ERR_INVALID; }
  SL2_HIP(hipSetDevice(e->device));
  { int rc = prepare_destination(e, false); if (rc != SL2_OK) return rc; }
  { int rc = launch_unpack(e, seq0, nseq, nullptr, 0, e->stream); if (rc != SL2_OK) return rc; }
  return settle_destination(e);
}

}  // extern "C"
