// Engine-internal declarations shared by the HIP translation units.
// gfx950 (MI355X / CDNA4) only; wavefront = 64.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/scenelib2_amd.h"
#include "sl2_math.hpp"
#include "sl2_seq_arrays.hpp"
#include "sl2_step_plan.hpp"
#include "sl2_update_plan.hpp"

namespace sl2 {

void set_error(const std::string& s);
const char* hip_err_text(hipError_t e);

#define SL2_HIP(call)                                                                          \
  do {                                                                                         \
    hipError_t _e = (call);                                                                    \
    if (_e != hipSuccess) {                                                                    \
      char _buf[512];                                                                          \
      snprintf(_buf, sizeof(_buf), "%s:%d: %s -> %s", __FILE__, __LINE__, #call, hipGetErrorString(_e)); \
      sl2::set_error(_buf);                                                                    \
      return SL2_ERR_HIP;                                                                      \
    }                                                                                          \
  } while (0)

// feature flag bits (f_flags)
enum : int {
  FF_ACTIVE = 1,      // slot holds a live feature
  FF_SCHEDULED = 2,   // scheduled_for_termination_flag_
  FF_SELECTED = 4,    // selected_flag_
  FF_SUCCESS = 8,     // successful_measurement_flag_
  FF_VISIBLE = 16,    // passed visibility_test in the last selection
  FF_USED = 32,       // slot was ever used (deleted features keep FF_USED)
  FF_PARTIAL = 64,    // label reserved by a partially initialised feature (its 6 states live at ppos + 6 k, k = its partial slot)
};

// feature initialisation (one partially initialised feature per sequence)
constexpr int kMaxParticles = 1024;      // upper bound of params.number_of_particles (k_map_particles: one thread per particle)
// Large search windows are cut into UNITS of a few bands (32 x 16 candidate positions each) that any wavefront of the search
// launch may take (sl2_search.hip: m4_big_windows).  sl2_engine::srch_big, ints: [0] units allocated this step (k_select),
// [1] windows shared out in the last completed step (sl2_get_step_work), [2] next unit to hand out, [3] windows shared out this
// step; then per unit: its entry (sequence, selected position, first unit of its window, units of its window), the count
// of finished units of the window (kept at the window's first unit) and its partial result (8 ints).
// Default threshold: 8 bands at 320 x 240 (150 bands a frame; mapping workload, step: 0.734 ms never, 0.687 at 24, 0.665 at 8,
// 0.661 at 4), the same twentieth of the frame at other sizes - what is shared out must be the rare window that is far larger
// than the rest, not the typical one: at 1280 x 720 x 500 features a threshold of 8 bands listed 8192 windows a step and
// the 2048 trailing workgroups became the search (2.19 against 1.24 ms, profiles/r04_search_shared_ab.txt).
constexpr int kSrchSplitDefault = 8;
__host__ __device__ inline int srch_split_default(int width, int height) {
  const int frame_bands = ((width + 31) / 32) * ((height + 15) / 16);
  const int t = frame_bands * kSrchSplitDefault / 150;
  return t > kSrchSplitDefault ? t : kSrchSplitDefault;
}
constexpr int kSrchBigUnits = 16384;                  // units per step and sequence group (a 320 x 240 window: 38); windows beyond stay with their own wavefront
constexpr int kSrchBigSlots = 64;                     // units per window at most: its partial results are combined by one wavefront, a lane each
constexpr int kSrchBigMinBands = 4;                   // bands per unit at least
constexpr int kSrchSharedNu = -(1 << 30);             // the width a shared window's record carries (srch_sel[..][4]; the true one: [14])
constexpr int kSrchBigEntries = 4;                    // int offsets into srch_big
constexpr int kSrchBigDone = kSrchBigEntries + 4 * kSrchBigUnits;
constexpr int kSrchBigParts = kSrchBigDone + kSrchBigUnits;
constexpr int kSrchBigInts = kSrchBigParts + 8 * kSrchBigUnits;
// seq_time, the per-sequence time record (sl2_engine::seq_time): the places of its kSeqTimeDoubles doubles
constexpr int kSeqTimeNominal = 0, kSeqTimeOwed = 1, kSeqTimeUsed = 2, kSeqTimeCatchUp = 3;
// seq_cam, the per-sequence camera calibration (sl2_engine::seq_cam): the places of its kSeqCamDoubles doubles - one 64-byte line;
// [6] and [7] are spare and stay 0.  sd is kept as a double: CameraParams::sd only ever enters cam.sd * (1.0 + ratio), an exact conversion.
constexpr int kSeqCamFku = 0, kSeqCamFkv = 1, kSeqCamU0 = 2, kSeqCamV0 = 3, kSeqCamKd1 = 4, kSeqCamSd = 5;
static_assert(kSeqCamDoubles * sizeof(double) == 64, "one cache line per sequence");
__host__ __device__ inline int srch_unit_bands(int bands) { const int g = (bands + kSrchBigSlots - 1) / kSrchBigSlots; return g > kSrchBigMinBands ? g : kSrchBigMinBands; }
// Partially initialised features: up to kMaxPartial per sequence (params.max_features_to_init_at_once, monoslam.cpp:163-167).
// part_i / part_d = the per-SEQUENCE record: feature_init_info_vector_.size(), the partial slots in the vector's order (a
// conversion or deletion erases an entry, the later ones move up), the image selection and the counters; ps_i / ps_d = one
// record per PARTIAL SLOT k (FeatureInitInfo): its six states live in columns ppos + 6 k of x / P.  (Their sizes, kPartInts /
// kPartDoubles and kPsInts / kPsDoubles, are in sl2_seq_arrays.hpp.)
constexpr int kMaxPartial = 4;
enum : int { kPartCount = 0, kPartOrder /* kMaxPartial ints */, kPartUU = 5, kPartVV, kPartRegionValid,
             kPartRegion /* 4 ints */, kPartInitialised = 12, kPartConverted, kPartDeleted, kPartCreated };
enum : int { kPsActive = 0, kPsLabel /* the feature SLOT that holds its label */, kPsAttempts, kPsNp, kPsMaking };
constexpr int kCholBlock = 32;       // block size of the blocked Cholesky / forward substitution
constexpr int kPatchPackedOffset = 128;   // where the packed form of a stored template starts (kPatchStride, sl2_seq_arrays.hpp)

// XCD-aware block -> (sequence, tile) mapping.  MI355X dispatches workgroup L to XCD L % 8 and
// every XCD has its own 4 MB L2; all tiles of one sequence share that sequence's operands
// (V^T, L, the frame), so they are placed on ONE XCD: the grid is 1-D with
// tiles * roundup(B, 8) blocks and block L works on sequence (L/8/tiles)*8 + L%8, tile (L/8)%tiles.
// (Placement is a speed matter only; any mapping is correct.)
constexpr int kXcds = 8;
inline int xcd_grid(int tiles, int B) { return tiles * round_up(B, kXcds); }
#if defined(__HIPCC__)
__device__ __forceinline__ bool xcd_map(int tiles, int B, int* seq, int* tile) {
  const int L = blockIdx.x;
  const int xcd = L % kXcds, slot = L / kXcds;
  *seq = (slot / tiles) * kXcds + xcd;
  *tile = slot % tiles;
  return *seq < B;
}
#endif

#if defined(__HIPCC__)
// The camera of sequence b, built in registers: its six intrinsics from the sequence's line of seq_cam, the geometry from the
// engine.  Called with a workgroup-uniform b the address is uniform too and the line arrives by scalar loads, in the SGPRs the
// by-value kernel argument used to occupy.  Nothing is precomputed: the models see the same six numbers as before.
__device__ __forceinline__ CameraParams load_cam(const double* __restrict__ seq_cam, int b, int width, int height) {
  const double* rec = seq_cam + (size_t)b * kSeqCamDoubles;
  CameraParams cam;
  cam.width = width; cam.height = height;
  cam.fku = rec[kSeqCamFku]; cam.fkv = rec[kSeqCamFkv]; cam.u0 = rec[kSeqCamU0]; cam.v0 = rec[kSeqCamV0];
  cam.kd1 = rec[kSeqCamKd1]; cam.sd = (int)rec[kSeqCamSd];
  return cam;
}
#endif

struct KernelTimer {
  std::string name;
  double total_ms = 0.0;
  int64_t launches = 0;
};
struct PendingEvent {
  int timer;
  hipEvent_t start, stop;
};

}  // namespace sl2

// The opaque engine object of the C ABI.  Its per-sequence device arrays (x, P, patch ... me_desc) are the members of
// sl2::SeqArrays, listed and documented in sl2_seq_arrays.hpp.
struct sl2_engine : sl2::SeqArrays {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  sl2::CameraParams cam;      // the camera of sl2_create: the image geometry of every sequence, and the calibration each one starts with (seq_cam)
  sl2_params prm;
  int B = 0;         // sequences
  int N = 0;         // feature capacity per sequence
  int ld = 0;        // leading dimension of x / P / At / Vt rows (>= 13 + 3N + 1, multiple of 64)
  int nsel_max = 0;  // max features measured per frame
  int mld = 0;       // leading dimension of the innovation system (>= 2 nsel_max, multiple of 32)
  int nblk_max = 0;  // mld / 32
  long long steps_done = 0;
  // The dense update's variants: 1 = the product's kernels, 0 = the superseded ones (TEST build).  Which kernel a variant - or
  // any knob of the update below - selects at which size is make_update_plan's to say (sl2_update_plan.hpp), nobody else's.
  int chol_variant = 1;       // factorisation: CholForm
  void* chol_trace = nullptr; // development only (SL2_CHOL_TRACE builds): per-wave cycle stamps of k_chol_fused4
  int build_variant = 1;      // A and S: BuildForm
  int fwd_variant = 1;        // forward substitution: FwdForm
  // ---- feature initialisation ----
  int ppos = 0;                          // first column of the partial features' states (13 + 3N); slot k at ppos + 6 k
  int kpart = 1;                         // partial slots per sequence: params.max_features_to_init_at_once, 1 .. kMaxPartial
  int pcap = 128;                        // particle slots per partial feature: roundup(params.number_of_particles, 64)
  double* score_map = nullptr;           // [B][kpart][H][W] score cache of an OVERSIZED multi-ellipse search (allocated on first use)
  int* me_big_list = nullptr;            // [B * kpart] (sequence, partial slot) jobs too large for the one-workgroup form, this step
  int* me_big_count = nullptr;           // [1]
  bool mapping_used = false;
  int* init_uv = nullptr;                // [B][2] pixel selections of sl2_initialise_feature (allocated on first use)
  // ---- whole-step HIP graphs (small batches are launch-bound: ~12 kernels per step) ----
  struct StepGraph { const void* frames; size_t stride; sl2::StepPlan plan; hipGraphExec_t exec; };   // a captured step: what it bakes in is its key
  bool graph_mode = false;
  std::vector<StepGraph> step_graphs;
  long long graph_captures = 0;   // steps captured so far (TEST build: sl2_debug_graph_captures - a setter that says it drops no captured step is held to it)
  int build_split = 0;        // development switches (TEST build only: SL2_BUILD_SPLIT, SL2_SCORE_THREADS, SL2_NO_KSPLIT read
  int score_threads = 0;      // once at sl2_create): 0 = the engine's own choice
  int no_ksplit = 0;
  int panel_from = 16;        // systems of more 32-blocks than this are factored panel-wise (launch_chol_panels) ...
  int group_from = sl2::kFwdLdsMaxBlocks;   // ... and substituted in groups of eight block rows (launch_fwdsub_grouped)
  int fwd_group = 8;          // block rows per group of the grouped substitution (TEST build: SL2_FWD_GROUP = 4 | 8)
  int chol_panel = 8;         // 32-blocks per panel of the large-map Cholesky: 8 (256 columns; 4.3 ms against 5.05 with 4 at
                              // 512 x n = 1513, profiles/r03_c5_chol_panel_ab.txt); TEST build: SL2_CHOL_PANEL = 4 | 8
  int build_ahead = 1;        // 1 = launches of one workgroup per sequence, ld <= 1024, take k_build_AS_ahead; TEST build: SL2_BUILD_AHEAD=0 keeps k_build_AS
  int build_lds_min = 0;     // minimum dynamic LDS bytes per k_build_AS workgroup (caps the workgroups a CU takes; TEST build: SL2_BUILD_LDS_MIN)
  int search_lds_pad = 0;     // extra dynamic LDS bytes per k_search_mfma workgroup (TEST build: SL2_SEARCH_LDS_PAD): an occupancy probe
  int search_chunk = 0;       // selected positions per wavefront of k_search_mfma (TEST build: SL2_SEARCH_CHUNK); 0 = the engine's own choice
  int search_variant = 1;     // 0 = exact kernel (one candidate per lane), 1 = int8 matrix-core walk (default)
  // How large the live maps are, known on the host WITHOUT a synchronisation (the choice of the step's kernels): finalize
  // publishes the batch's maximum of n_slots per step to pinned memory (sl2_frontend_dev.hpp: finalize_body); exact values
  // are taken wherever a call synchronises anyway (sl2_add_known_features, the "initialise feature" buttons).
  int* slots_max_dev = nullptr;                  // [2] device: maxima of the steps in flight (step parity)
  unsigned long long* slots_mail = nullptr;      // pinned + mapped host word: (step << 32) | max n_slots of the step before it
  unsigned long long* slots_mail_dev = nullptr;  // its device address
  unsigned long long* parts_mail = nullptr;      // the word after it, one-sequence engines: (steps completed << 32) | partially initialised features left by k_map_update
  unsigned long long* parts_mail_dev = nullptr;
  int place_candidates = 0;                      // sl2_create's placement of the large matrices (sl2_engine.hip: place_large_matrices): sets probed,
  float place_syrk_ms[2] = {0, 0};               // k_syrk on the kept (P, V^T) and on the slowest pair probed
  float place_kept_ms[4] = {0, 0, 0, 0};         // probe time of the kept P, V^T, A^T, S and of the slowest candidate of each size
  float place_worst_ms[3] = {0, 0, 0};
  long long parts_block_step = -1;               // a step of this index must not trust parts_mail (a feature was initialised by hand since)
  int slots_exact = 0;                           // max n_slots over the batch when last read back ...
  long long slots_exact_step = 0;                // ... and steps_done at that point
  int step_fusion = 1;        // small maps (sl2_small.hip: ld <= 128, one 32-row innovation block) step in three launches instead of ten; 0 = never (sl2_set_step_fusion)
  int search_split = sl2::kSrchSplitDefault;   // windows of at least this many 32 x 16 bands are shared out over wavefronts (0 = never); sl2_create: srch_split_default, then sl2_set_search_split
  // ---- large search windows (round 4): the step's units of work for every wavefront of k_search_mfma (layout: kSrchBig* above) ----
  int* srch_big = nullptr;    // per sequence GROUP (allocated by build_groups)
  // ---- three rows of SL2_SEQ_ARRAYS that are engine state of a sequence, in no sequence blob ----
  // step_mark (sl2_get_step_stats, sl2_stats.hip): 1 = the sequence took part in the last make_measurements
  // (k_search_score / k_small_back write it next to m_gate: 1 for an active sequence, 0 for a paused one) and has not been loaded,
  // copied in or reset since (k_seq_unpack clears it).
  // seq_time (sl2_set_delta_t): [0] the sequence's nominal time step (params.delta_t after sl2_create), [1] time owed
  // by predicts a paused sequence skipped (catch-up on only), [2] the step its last predict used (the speed gate of k_map_find
  // divides by it), [3] the catch-up switch, 0 or 1.  Read and written by predict_body and the paused branch of its two kernels;
  // the setters write it with kernels on the engine's stream, so a captured step reads it as data.
  // seq_cam (sl2_set_cameras): fku, fkv, u0, v0, kd1, sd of the sequence (the sl2_create camera's until
  // sl2_set_cameras), two spare words.  Read through load_cam by every step kernel that projects or unprojects; written only by
  // the setter's kernel on the engine's stream, so a captured step reads it as data.  A sequence blob RECORDS it (header.camera)
  // and a load checks it, but nothing but the setter writes it.  cams_host (root only) is the host's copy of what the setters
  // queued so far: sl2_get_cameras and the checkpoint checks answer from it without waiting for the device.
  std::vector<sl2_camera> cams_host;
  void* stats_host = nullptr;      // pinned + mapped host memory the host form of sl2_get_step_stats fills: [B] records (first use)
  void* stats_host_dev = nullptr;  // its device-side address

  // ---- engine-owned staging of the state accessors (no allocation per call; released by sl2_destroy) ----
  void* snap_stage = nullptr;     // device: the packed blob of sl2_snapshot
  void* snap_host = nullptr;      // pinned + mapped host memory the blob is streamed into (what sl2_snapshot returns)
  void* snap_host_dev = nullptr;  // its device-side address
  size_t snap_cap = 0;            // bytes of the blob area; the completion word the kernel writes last sits right behind it
  unsigned long long snap_ticket = 0;
  void* snapb_stage = nullptr;    // device: the packed blobs of the host form of sl2_snapshot_batch (first use: bound x nseq; grown on demand)
  size_t snapb_stage_bytes = 0;
  void* snapb_aux = nullptr;      // device: its offsets [B + 1] (uint64), then its cursors [B][2] (int32)
  void* snapb_aux_host = nullptr; // pinned host memory of the same layout: the cursors on their way in, the offsets on their way out
  void* ovl_lists = nullptr;      // device: the draw lists of the host forms of sl2_overlay_items, sl2_scene_items and sl2_world_items and of sl2_draw_overlays,
                                  // sl2_draw_rectified and sl2_draw_world: items, counts, marked labels, views, extents (sl2_display.hpp: ListStage; first use, grown on demand)
  size_t ovl_lists_bytes = 0;
  void* ovl_images = nullptr;     // device: host frames on their way in, grey frames and images on their way out of sl2_draw_overlays, sl2_rectify_frames,
                                  // sl2_draw_rectified and sl2_draw_world (sl2_display.hpp: draw_call; first use, grown on demand)
  size_t ovl_images_bytes = 0;
  void* acc_dev = nullptr;        // device scratch of the get / set accessors (grown on demand)
  size_t acc_dev_bytes = 0;
  void* acc_host = nullptr;       // pinned host scratch of the same calls
  size_t acc_host_bytes = 0;
  void* ckpt_stage = nullptr;     // device: the blobs of one chunk of sl2_save_sequences / sl2_load_sequences / sl2_copy_sequences (grown on demand, bounded)
  size_t ckpt_stage_bytes = 0;
  hipEvent_t ckpt_event = nullptr;   // orders two engines' streams in sl2_copy_sequences

  uint8_t* frames_buf = nullptr;  // [B][W*H] staging for host frames
  const uint8_t* cur_frames = nullptr;
  size_t cur_stride = 0;

  // profiling
  bool profiling = false;
  int profile_level = 2;
  std::string profile_focus;  // level 1: bracket only these kernels (",name,name,"); empty = the four major ones
  std::vector<sl2::KernelTimer> timers;
  std::vector<sl2::PendingEvent> pending;
  std::vector<hipEvent_t> event_pool;

  // ---- sequence groups: the batch is split into G contiguous groups, each stepped on its own
  // HIP stream, so that the latency-bound kernels of one group (blocked Cholesky, selection,
  // bookkeeping) overlap with the throughput-bound kernels of another (SYRK, substitution, search).
  // A group is a shallow copy of the root engine whose per-sequence pointers are offset (sl2_seq_arrays.hpp: seq_arrays_view).
  sl2_engine* root = nullptr;           // self for the root object
  std::vector<sl2_engine*> groups;      // root only
  int group_first = 0;                  // first sequence of this group
  hipEvent_t fork_event = nullptr;

  int timer_id(const char* name);
  void prof_begin(int id, hipStream_t st);
  void prof_end(hipStream_t st);
  int fold_events();
  int sync_all();
};

namespace sl2 {

// What a kernel receives of an engine or a group: the table of its per-sequence arrays, by value, beside a struct of scalars.
inline const SeqArrays& seq_arrays(const sl2_engine* e) { return *e; }

// RAII-less helper: bracket a launch with events when profiling is on.
struct LaunchScope {
  sl2_engine* e;
  bool on;
  size_t slot = 0;
  // level 1 = only the roofline kernels (cheap: 4 event pairs per step), level 2 = every launch
  static bool wanted(const sl2_engine* r, const char* name, bool major) {
    if (!r->profiling) return false;
    if (r->profile_level >= 2) return true;
    if (!major) return false;
    if (r->profile_focus.empty()) return true;
    return r->profile_focus.find(std::string(",") + name + ",") != std::string::npos;
  }
  LaunchScope(sl2_engine* eng, const char* name, bool major = false) : e(eng), on(wanted(eng->root, name, major)) {
    if (on) { e->root->prof_begin(e->root->timer_id(name), e->stream); slot = e->root->pending.size() - 1; }
  }
  ~LaunchScope() {
    if (on) hipEventRecord(e->root->pending[slot].stop, e->stream);
  }
};

// launchers implemented in the kernel translation units (all asynchronous on e->stream)
int launch_predict(sl2_engine* e);
int launch_feature_prediction(sl2_engine* e);
int launch_select(sl2_engine* e, int n);
int launch_search(sl2_engine* e);            // the search kernel, then k_search_score
int launch_search_kernel(sl2_engine* e);     // the search kernel alone (the fused small-map step scores in k_small_back)
int launch_search_score(sl2_engine* e);
int launch_small_front(sl2_engine* e, int n);                 // predict + feature prediction + selection in one launch
int launch_small_back(sl2_engine* e, int save_trajectory, int panel_w);   // (GroupPlan::panel_w) scoring + EKF update + normalise / delete / symmetrise in one launch
int launch_update(sl2_engine* e);
// the phases launch_update walks, a translation unit each (sl2_update_build.hip, sl2_update_chol.hip, sl2_update_fwdsub.hip,
// sl2_update_syrk.hip): the plan's form of the phase, or kNoProductForm where the unit holds no kernel for it
constexpr int kNoProductForm = -1;
int launch_build(sl2_engine* e, const UpdatePlan& p);
int launch_factor(sl2_engine* e, const UpdatePlan& p);
int launch_substitute(sl2_engine* e, const UpdatePlan& p);
int launch_product(sl2_engine* e);
int launch_panel_solve(sl2_engine* e, int pb, int p0, int c0, int ntile, int nb);   // sl2_update_fwdsub.hip, for the panel-wise Cholesky: X = S[below][panel] L_dd^-T
int launch_syrk_on(sl2_engine* e, const double* Vt, double* P);
UpdateShape update_shape(const sl2_engine* e);   // sl2_ekf_update.hip: what make_update_plan takes of an engine
// sl2_update_testing.hip (the TEST library only): the superseded forms
int launch_build_two_pass(sl2_engine* e, int threads);
int launch_chol_per_block(sl2_engine* e);
int launch_fwdsub_reread(sl2_engine* e);
int launch_finalize(sl2_engine* e, int save_trajectory);
int launch_mapping(sl2_engine* e, const TailPlan& tp);
int launch_manual_init(sl2_engine* e, const int* d_uv);
int launch_auto_init(sl2_engine* e);
int launch_compact_slots(sl2_engine* e, int need, bool honour_mask = false);   // sl2_mapping.hip: retired slots squeezed out when a sequence lacks room for `need` more features (honour_mask: the launch of a step, which leaves paused sequences alone)
// sl2_engine.hip, for sl2_checkpoint.hip: what a call owes the engine when it replaces sequences under it
int checkpoint_refresh_slots(sl2_engine* e);         // refresh_slots_exact
int checkpoint_drop_graphs(sl2_engine* e);           // drop_step_graphs
int checkpoint_enable_mapping(sl2_engine* e);        // enable_feature_initialisation
void release_checkpoint_staging(sl2_engine* e);      // sl2_checkpoint.hip (sl2_destroy)
int write_grey_image(const char* path, const uint8_t* px, int w, int h);   // sl2_ingest.hip (PGM / PNG)

}  // namespace sl2
