/*
 * scenelib2_amd — C ABI of the MI355X-native MonoSLAM per-frame engine.
 *
 * The reference (hanmekim/SceneLib2) has no plugin/FFI layer: its boundary is the
 * public C++ class SceneLib2::MonoSLAM (scenelib2/monoslam.h:69-219) used by
 * examples/MonoSlamSceneLib1.cpp:132-142.  This header is the C-ABI a maintainer
 * binds instead: plain pointers and sizes, int status codes,
 * no exceptions, no torch/Eigen/OpenCV types.  Each entry point cites the
 * reference interface it replaces (paths relative to the reference's scenelib2/).
 *
 * One engine = B independent image sequences ("batch"), each an independent
 * MonoSLAM instance with its own state vector, covariance, map and templates,
 * stepped together on one HIP stream of one GPU.  All *_dev pointers are device
 * pointers valid on the engine's device; host pointers are plain host memory.
 * All matrices crossing the ABI are row-major FP64 unless stated.
 *
 * Threading: one engine per host thread / stream; calls are asynchronous on the
 * engine's stream unless they return data to host memory (those synchronise).
 */
#ifndef SCENELIB2_AMD_H
#define SCENELIB2_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Version of this interface.  Bumped whenever an entry point changes meaning or a buffer it fills changes size; the
 * library reports the version it was built from through sl2_api_version(), so a caller compiled against an older header can
 * tell.  History: 1 = round 1; 2 = sl2_get_step_work fills 11 doubles, search variants 0-3; 3 = sl2_get_step_work fills 12
 * doubles (out[11] = candidate tiles), search variants renumbered (1 = int8 matrix-core walk, 0 = exact kernel; 2 and 3 are
 * gone and return SL2_ERR_INVALID), sl2_set_update_variant accepts only (1, 1) outside the TEST build; 4 = sl2_get_step_work
 * takes the capacity of the caller's array, sl2_snapshot / sl2_snapshot_capacity, several partially initialised features per
 * sequence (max_features_to_init_at_once > 1), sl2_get_partial_feature takes the index of the partial feature; 5 = sl2_ingest_next
 * uploads on a stream of its own, one frame ahead (or hands a small batch out in place): its `stream` argument is the stream the
 * frames are CONSUMED on, not the one the copy is queued on; sl2_set_update_variant no longer takes chol_variant 2; new:
 * sl2_set_step_fusion, sl2_get_stream, sl2_ingest_set_zero_copy; scenelib2_amd_comm.h.  Additions within 5: sl2_save_sequences,
 * sl2_load_sequences, sl2_copy_sequences, sl2_reset_sequences, sl2_sequence_blob_capacity, sl2_sequence_blob_layout;
 * sl2_snapshot_header.sequence_steps (taken from reserved[]); sl2_set_active_sequences, sl2_get_active_sequences,
 * sl2_ingest_frame_counts, sl2_ingest_next_ragged; sl2_get_step_stats (sl2_step_stats); sl2_set_delta_t, sl2_get_delta_t,
 * sl2_set_pause_catch_up (the time step is the sequence's: sl2_params.delta_t is its initial value); sl2_set_cameras,
 * sl2_get_cameras (the calibration is the sequence's: the sl2_create camera is its initial value and the batch's image size);
 * sl2_converter_create, sl2_converter_destroy, sl2_converter_set_sources, sl2_converter_get_sources, sl2_convert_frames,
 * sl2_convert_frame_host, sl2_scale_camera (raw camera frames of any size and pixel format, in front of the step);
 * sl2_converter_set_filters, sl2_converter_get_filters, sl2_convert_frame_host_filtered (SL2_RESIZE_AREA: the exact box average
 * for cameras much larger than the engine's image); sl2_snapshot_batch, sl2_snapshot_bound, SL2_SNAP_*,
 * sl2_snapshot_header.omitted_sections (taken from reserved[]: the public state of a range of sequences in one call); sl2_overlay_items,
 * sl2_draw_overlays, sl2_draw_items_batch, sl2_draw_items_host, sl2_overlay_item_bound, sl2_overlay_item, SL2_ITEM_*,
 * SL2_OVERLAY_* (annotated frames: the raw-image display of GraphicTool::DrawRawAR as a draw list and a rasteriser);
 * SL2_ITEM_SEGMENT, sl2_rectify_frames, sl2_rectify_frame_host, sl2_scene_items, sl2_scene_item_bound, sl2_draw_rectified,
 * SL2_SCENE_* (the rectified view of GraphicTool::DrawRectifiedAR: a line primitive, the undistorted frame, the 3-D scene);
 * sl2_view, sl2_view_look_at, sl2_world_items, sl2_world_item_bound, sl2_draw_world, SL2_WORLD_*, sl2_pick_items_batch,
 * sl2_pick_items_host (the world view of GraphicTool::Draw3dScene from a free camera, and GraphicTool::Picker);
 * sl2_converter_set_map, sl2_converter_set_remaps, sl2_converter_get_remaps, sl2_remap_frame_host, SL2_REMAP_BORDER, sl2_lens,
 * SL2_LENS_*, sl2_lens_map_host, sl2_lens_pinhole_camera (the lens remap: OpenCV and fisheye cameras through a per-pixel map);
 * sl2_frame_monitor_create, sl2_frame_monitor_destroy, sl2_frame_monitor_set_gates, sl2_frame_monitor_get_gates,
 * sl2_frame_monitor_reset, sl2_examine_frames, sl2_frame_monitor_read, sl2_frame_stats_host, sl2_frame_verdict_host,
 * sl2_frame_stats, sl2_frame_gate, SL2_FRAME_* (the frame monitor: per-sequence frame statistics and a device-side gate in front
 * of sl2_set_active_sequences). */
#define SL2_API_VERSION 5

#define SL2_OK 0
#define SL2_ERR_INVALID 1   /* bad argument */
#define SL2_ERR_HIP 2       /* HIP runtime error (sl2_last_error() has the text) */
#define SL2_ERR_CAPACITY 3  /* feature / batch capacity exceeded */
#define SL2_ERR_NO_DEVICE 4 /* no HIP device: the engine has NO CPU fallback */

#define SL2_STATE_SIZE 13    /* MotionModel::kStateSize_, motion_model.cpp:44 */
#define SL2_POSITION_SIZE 7  /* MotionModel::kPositionStateSize_ */
#define SL2_PATCH_SIZE 11    /* MonoSLAM::kBoxSize_, monoslam.cpp:48 */
#define SL2_PATCH_BYTES 121

typedef struct sl2_engine sl2_engine;

/* Camera::SetCameraParameters(width,height,fku,fkv,u0,v0,kd1,sd) — camera.cpp:49-62.
 * cfg keys cam.* (data/SceneLib2.cfg:24-31); fku,fkv,u0,v0,sd are read as ints by
 * the reference (monoslam.cpp:1597-1602) but stored as doubles/ints as below. */
typedef struct sl2_camera {
  int32_t width, height;
  double fku, fkv, u0, v0, kd1;
  int32_t sd;
} sl2_camera;

/* cfg keys params.* (data/SceneLib2.cfg:59-69, monoslam.cpp:1583-1593) plus the two
 * hard-wired deletion constants (monoslam.cpp:1875-1876). */
typedef struct sl2_params {
  double delta_t; /* the initial time step of every sequence; sl2_set_delta_t gives a sequence its own */
  int32_t number_of_features_to_select;
  int32_t number_of_features_to_keep_visible;
  int32_t max_features_to_init_at_once;
  double min_lambda, max_lambda;
  int32_t number_of_particles;
  double standard_deviation_depth_ratio;
  int32_t min_number_of_particles;
  double prune_probability_threshold;
  int32_t erase_partially_init_feature_after_this_many_attempts;
  int32_t minimum_attempted_measurements_of_feature; /* 10 */
  double successful_match_fraction;                  /* 0.5 */
} sl2_params;

/* Per-feature record returned by sl2_get_features — the public members of
 * SceneLib2::Feature that GraphicTool / the example read (feature.h:78-142). */
typedef struct sl2_feature_info {
  int32_t label;                               /* Feature::label_ */
  int32_t active;                              /* 0 once delete_feature() removed it */
  int32_t selected_flag;                       /* Feature::selected_flag_ */
  int32_t successful_measurement_flag;         /* Feature::successful_measurement_flag_ */
  int32_t attempted_measurements_of_feature;   /* Feature::attempted_measurements_of_feature_ */
  int32_t successful_measurements_of_feature;  /* Feature::successful_measurements_of_feature_ */
  int32_t position_in_total_state_vector;      /* as the reference would report it (deleted features removed) */
  int32_t visible;                             /* visibility_test()==0 in the last auto_select_n_features */
  double y[3];                                 /* Feature::y_ */
  double h[2], z[2], nu[2];                    /* h_, z_, nu_ */
  double R;                                    /* R_ = R * I2 */
  double S[4];                                 /* S_ (2x2) */
  double dh_by_dxp[14];                        /* first 7 columns of dh_by_dxv_ (rest are zero) */
  double dh_by_dy[6];                          /* dh_by_dy_ (2x3) */
  double xp_org[7];                            /* xp_org_ */
  int32_t fully_initialised_flag;              /* Feature::fully_initialised_flag_ (0: the six-state ray of a partially initialised feature) */
  int32_t state_size;                          /* 3, or 6 while partially initialised */
  double y_direction[3];                       /* partially initialised: y_(3..5), the unit ray direction; else 0 */
} sl2_feature_info;

/* ------------------------------------------------------------------ lifecycle */

/* SL2_API_VERSION of the library that is loaded (compare with the header's). */
int sl2_api_version(void);
/* Number of HIP devices visible (0 => every other call fails with SL2_ERR_NO_DEVICE). */
int sl2_device_count(void);

/* Replaces `new MonoSLAM` + the object wiring of MonoSLAM::Init (monoslam.cpp:1852-1885)
 * for `batch` sequences with room for `max_features` features each.  `stream` is a
 * hipStream_t (NULL => the engine creates its own). */
/* Limits (SL2_ERR_CAPACITY): at most 676 feature slots per sequence (2048 state columns: one k_build_AS workgroup holds a
 * sequence's row of A^T) and 512 features measured per frame (number_of_features_to_select); the reference's feature_list_ is
 * unbounded.  BASELINE's largest configuration (500 features, 1513 states) is inside. */
int sl2_create(const sl2_camera* cam, const sl2_params* params, int batch, int max_features, int device,
               void* stream, sl2_engine** out);
void sl2_destroy(sl2_engine* e);
const char* sl2_last_error(void);
int sl2_synchronize(sl2_engine* e);
/* The hipStream_t the engine's steps are queued on (the one given to sl2_create, or the engine's own): what sl2_ingest_next and
 * the scenelib2_amd_comm.h calls want as their `stream`. */
void* sl2_get_stream(sl2_engine* e);
int sl2_batch(const sl2_engine* e);
int sl2_max_features(const sl2_engine* e);

/* xv_ and Pxx_ as MonoSLAM::Init sets them (monoslam.cpp:1881-1938): xv [nseq][13] in
 * the order r(3) q(w,x,y,z) v(3) omega(3); Pxx [nseq][13][13]. */
int sl2_set_vehicle_state(sl2_engine* e, int seq0, int nseq, const double* xv, const double* Pxx);
int sl2_get_vehicle_state(sl2_engine* e, int seq0, int nseq, double* xv, double* Pxx);

/* MonoSLAM::AddNewKnownFeature(y, xp, identifier) (monoslam.cpp:1278-1291 ->
 * Feature ctor feature.cpp:108-149), batched: `nfeat` features appended to each of
 * sequences [seq0, seq0+nseq).  y [nseq][nfeat][3], xp_org [nseq][nfeat][7],
 * patches [nseq][nfeat][121] = the 11x11 8-bit template the reference would
 * cv::imread from `identifier`.  Labels continue from next_free_label_; a sequence that lacks free slots first gets the slots
 * of its deleted features back (see SL2_STATUS_LABELS_EXHAUSTED below); SL2_ERR_CAPACITY if it still holds more than
 * max_features - nfeat live features.  The call is all or nothing as far as features go: when ANY sequence of the range
 * lacks room, no sequence gets a feature and no label is used up.  What a failing call may have done is give other
 * sequences their deleted features' slots back - a renumbering no accessor shows (slots are not part of the interface;
 * sl2_get_features(include_deleted) merely stops listing the deleted features).  A sequence with room is not touched.
 * The call may come between the seams of a step (sl2_kalman_filter_predict ... sl2_finish_step): the selection, the search
 * records, the measurements and the recorded positions (Q28) of the frame in progress follow their features to the new
 * slots.  A feature added behind sl2_auto_select_n_features joins the selection with the next frame, like the
 * reference's AddNewKnownFeature at that point. */
int sl2_add_known_features(sl2_engine* e, int seq0, int nseq, int nfeat, const double* y, const double* xp_org,
                           const uint8_t* patches);

/* Feature::Pyy_ of the first `nfeat` features of each sequence (feature.h:84): Pyy [nseq][nfeat][3][3].
 * AddNewKnownFeature leaves it zero (feature.cpp:134-135); a map whose features carry a prior
 * uncertainty (what feature initialisation produces, feature.cpp:241-244) is loaded with this. */
int sl2_set_feature_covariances(sl2_engine* e, int seq0, int nseq, int nfeat, const double* Pyy);

/* ------------------------------------------------------------------- stepping */

/* MonoSLAM::GoOneStep(frame, save_trajectory, enable_mapping) (monoslam.cpp:108-180)
 * for every sequence.  frames: [batch] images of width*height bytes, 8-bit single
 * channel, row pitch == width (Q25); seq_stride = bytes between consecutive
 * sequences' frames.  frames_on_device != 0 => `frames` is a device pointer
 * (zero-copy); otherwise host memory, copied H2D on the engine's stream.
 * enable_mapping != 0 runs the feature-initialisation tail (monoslam.cpp:152-170: AutoInitialiseFeature behind the
 * 0.2 m/s speed gate, MatchPartiallyInitialisedFeatures) with up to params.max_features_to_init_at_once <= 4 partially
 * initialised features in flight per sequence (the shipped value is 1; the six state columns of each are reserved at
 * sl2_create) and up to 1024 depth particles (params.number_of_particles; the shipped value is 100); other settings are
 * rejected with SL2_ERR_INVALID.  The reference's own arithmetic is kept for the position it records for later features
 * after a conversion (feature.cpp:254, Q28): it is misplaced whenever a feature converts in front of one that joined the map
 * after it - a second partially initialised feature, or a known feature added while one was in flight - and that feature's
 * dh_by_dy block then lands where the reference puts it.  SL2_STATUS_LABELS_EXHAUSTED = a sequence could
 * not take a new feature because all max_features slots hold live features. */
int sl2_go_one_step(sl2_engine* e, const uint8_t* frames, size_t seq_stride, int frames_on_device,
                    int save_trajectory, int enable_mapping);

/* Stepping a subset of the batch.  Every sequence has one byte of engine state, `active`, on the device: all ones after
 * sl2_create.  A step issued while active[b] == 0 - sl2_go_one_step in every form it takes (fused or not, graph replay, sequence
 * groups, large maps, the feature-initialisation tail) and each of the five seams below - leaves sequence b exactly as it
 * was, bit for bit: state and covariance, templates, flags, counters, the per-frame values the accessors read, partially
 * initialised features and their particles, the drand48 stream, the trajectory store and the status bits.  The engine's step
 * clock is shared, so three things do move: the position log gets one more entry that repeats the unchanged camera position
 * (it stays aligned with the engine's steps), the sequence's own step count (sl2_sequence_blob_header.sequence_steps,
 * sl2_snapshot_header.sequence_steps) stands still while the engine's advances, and the sequence's map size still counts
 * towards the engine's choice of step kernels.  A sequence that is resumed predicts over one nominal step of its own (sl2_set_delta_t) by
 * default, as the reference does when it is handed the next frame, or over the nominal step plus the time owed by the predicts
 * it skipped with catch-up on (sl2_set_pause_catch_up).  The bytes of a paused sequence's frame are not read.
 * The mask is not part of a sequence blob (it belongs to the engine that steps, not to the sequence) and is left alone by
 * sl2_load_sequences / sl2_copy_sequences / sl2_reset_sequences.  It is consulted by STEPS only: sl2_add_known_features,
 * sl2_set_vehicle_state, sl2_set_feature_covariances, sl2_delete_features, sl2_initialise_feature,
 * sl2_initialise_auto_feature and checkpoint load / copy / reset act on the sequences they are given whatever the mask says.
 * Change it between steps; changing it between the seams of one step is undefined.
 *
 * sl2_set_active_sequences: active[i] != 0 = sequence seq0 + i takes part in the steps issued after this call.  on_device == 0:
 * `active` is host memory of any kind (pageable, pinned, registered) and is consumed before the call returns; on_device != 0:
 * a device pointer, read by a copy kernel on the engine's stream (keep it alive and unchanged until the stream has passed
 * this point).  Either way the change is ordered on the engine's stream: after every step already queued, before the next one.
 * The call never waits for the device and drops no captured step (the mask is data a replayed graph reads, not part of
 * its key).  SL2_ERR_INVALID: a range outside the batch or a null pointer. */
int sl2_set_active_sequences(sl2_engine* e, int seq0, int nseq, const uint8_t* active, int on_device);
/* sl2_get_active_sequences: the mask as the steps queued so far leave it (1 / 0 per sequence), to host memory.  Synchronises. */
int sl2_get_active_sequences(sl2_engine* e, int seq0, int nseq, uint8_t* active);

/* The time step is the sequence's.  Every sequence has a record of engine state on the device: its nominal time step
 * (sl2_params.delta_t after sl2_create), the time owed by predicts it skipped while paused, and the step its last predict used.
 * A predict - sl2_kalman_filter_predict and sl2_go_one_step in every form - moves sequence b over nominal + owed, notes that as
 * the step it used and clears what was owed; with nothing owed that is the nominal step, bit for bit.  The feature-
 * initialisation tail divides the camera's displacement by the step the last predict used - the nominal step while the sequence
 * has not predicted in this engine yet - (the 0.2 m/s speed gate) and looks
 * ten NOMINAL steps ahead for its search region.  Like the mask, the record belongs to the engine that steps: it is in no
 * sequence blob and sl2_load_sequences / sl2_copy_sequences / sl2_reset_sequences leave it alone.
 *
 * sl2_set_delta_t: dt[i] becomes the nominal step of sequence seq0 + i, and what that sequence was owed is cleared.  on_device
 * == 0: `dt` is host memory of any kind and is consumed before the call returns; on_device != 0: a device pointer, read by a
 * copy kernel on the engine's stream (keep it alive and unchanged until the stream has passed this point).  Either way the
 * change is ordered on the engine's stream: after every step already queued, before the next one.  The call never waits for the
 * device and drops no captured step (the record is data a replayed graph reads, not part of its key).  The mask is not
 * consulted: a paused sequence can be given its time step before it resumes.  SL2_ERR_INVALID, and nothing changed: a range
 * outside the batch, a null pointer, or - host form - any value that is not finite or is <= 0.  The device form cannot refuse:
 * it SKIPS such entries, and those sequences keep the step they had. */
int sl2_set_delta_t(sl2_engine* e, int seq0, int nseq, const double* dt, int on_device);
/* sl2_get_delta_t: the record as the steps and setters queued so far leave it, to host memory: the nominal step, the time owed
 * and the step the last predict used (0 before the first) of each sequence.  owed and last_used may be NULL.  Synchronises. */
int sl2_get_delta_t(sl2_engine* e, int seq0, int nseq, double* dt, double* owed, double* last_used);
/* sl2_set_pause_catch_up: enabled != 0 = from now on every predict a paused sequence sits out adds its nominal step to what
 * the sequence is owed, so the predict that resumes it covers the whole gap (a camera that dropped frames); this one word is the
 * only thing of a paused sequence a step then moves.  0 (the default) = a paused sequence is owed nothing, and what any
 * sequence was owed is cleared.  For the whole batch, by a kernel on the engine's stream: ordered like sl2_set_delta_t, never
 * waits, drops no captured step. */
int sl2_set_pause_catch_up(sl2_engine* e, int enabled);

/* The camera calibration is the sequence's.  The camera given to sl2_create fixes the image size of the whole batch (frame
 * strides, search tiles and the detector's tiling depend on it) and is the calibration every sequence starts with; the six
 * intrinsics fku, fkv, u0, v0, kd1, sd are then a record per sequence on the device, read by every kernel of a step that
 * projects or unprojects, so one batch serves physically different cameras of one image size.
 *
 * sl2_set_cameras: cams[i] becomes the calibration of sequence seq0 + i for every step issued after the call.  `cams` is host
 * memory of any kind and is consumed before the call returns.  The change is ordered on the engine's stream: after every step
 * already queued, before the next one.  The call never waits for the device and drops no captured step (the record is data
 * a replayed graph reads, not part of its key).  The mask is not consulted: a paused sequence can be given its camera before it
 * resumes.  SL2_ERR_INVALID, and NOTHING changed in any sequence of the range: a range outside the batch, a null pointer, any
 * cams[i] whose width / height differ from the engine's, any of fku, fkv, u0, v0, kd1 that is not finite, fku == 0 or
 * fkv == 0, sd < 0.
 * Sequence blobs record the calibration (sl2_sequence_blob_header.camera is the SEQUENCE's) and sl2_load_sequences /
 * sl2_copy_sequences refuse a blob whose camera differs from the destination sequence's: a map continued under another
 * calibration would be silently wrong.  They, and sl2_reset_sequences, never change a calibration: to move a sequence, set the
 * destination's camera first. */
int sl2_set_cameras(sl2_engine* e, int seq0, int nseq, const sl2_camera* cams);
/* sl2_get_cameras: the calibration of each sequence as the setters called so far leave it, with the engine's width / height.
 * Answered from the engine's host-side copy: does NOT synchronise. */
int sl2_get_cameras(sl2_engine* e, int seq0, int nseq, sl2_camera* cams);

/* The seams of GoOneStep, individually callable (same order as the reference):
 *   Kalman::KalmanFilterPredict(monoslam,u=0)            kalman.cpp:50-69
 *   MonoSLAM::auto_select_n_features(n)                  monoslam.cpp:187-254
 *   MonoSLAM::make_measurements(image)                   monoslam.cpp:336-359
 *   Kalman::KalmanFilterUpdate(monoslam)+normalise_state kalman.cpp:72-119, monoslam.cpp:616-637
 *   delete_bad_features + symmetrise                     monoslam.cpp:141-150
 */
/* MonoSLAM::InitialiseFeature(frame) (monoslam.cpp:1211-1235; the "initialise manual feature" button of
 * examples/MonoSlamSceneLib1.cpp:191-192, after a mouse click set uu_ / vv_): for every sequence s with uv[2 s] >= 0 a
 * partially initialised feature is created at pixel (uu_, vv_) = (uv[2 s], uv[2 s + 1]) of that sequence's frame - the
 * 11 x 11 patch copied from the frame, the semi-infinite line from the current pose, number_of_particles depth hypotheses
 * - exactly as the feature-initialisation tail of sl2_go_one_step creates one.  Later steps match and convert it
 * (MatchPartiallyInitialisedFeatures runs in every step from now on, like monoslam.cpp:167).  uv: host [batch][2], consumed
 * before the call returns (pageable, pinned or registered memory alike).
 * created: host [batch], may be NULL (the kernels then stay asynchronous); 1 = a feature was created.  It is NOT created -
 * and the reference would have created it - when the sequence already has a partially initialised feature (this engine
 * carries one at a time, the shipped max_features_to_init_at_once = 1), when the patch would leave the frame (the
 * reference reads out of bounds), or when the label slots are exhausted (SL2_STATUS_LABELS_EXHAUSTED). */
int sl2_initialise_feature(sl2_engine* e, const uint8_t* frames, size_t seq_stride, int frames_on_device, const int32_t* uv,
                           int32_t* created);
/* MonoSLAM::InitialiseAutoFeature(frame) (monoslam.cpp:1535-1541, the "initialise auto feature" button): AutoInitialiseFeature
 * with zero control input for every sequence - FindNonOverlappingRegion (consumes the sequence's drand48 stream), the
 * Shi-Tomasi detector, the 20000 score threshold, then the creation above - without the speed and visible-feature gates
 * of GoOneStep.  created as above. */
int sl2_initialise_auto_feature(sl2_engine* e, const uint8_t* frames, size_t seq_stride, int frames_on_device, int32_t* created);
/* MonoSLAM::SavePatch (monoslam.cpp:1551-1572): writes Feature::patch_ of the feature with this label (the reference saves
 * the marked feature to "patch.png").  ".pgm" writes a binary PGM, any other name an 8-bit greyscale PNG.  Synchronises. */
int sl2_save_patch(sl2_engine* e, int seq, int label, const char* path);

/* Split the batch into `groups` contiguous sequence groups, each stepped on its own HIP stream
 * (latency-bound kernels of one group overlap throughput-bound kernels of another).  Default 1
 * (measured on MI355X: no gain from 2, a loss from 4+ at batch 1024).  The library never reads the environment: the
 * SL2_* development switches exist in the TEST build (libscenelib2_amd_test.so) only. */
int sl2_set_groups(sl2_engine* e, int groups);
/* Whole-step HIP graphs: when enabled, sl2_go_one_step with device-resident frames captures its launches once per
 * (frame buffer, flags) and replays the graph (at batch 1 the step is launch-bound: ~12 kernels).  Off by default;
 * ignored while per-kernel profiling is on or with more than one sequence group. */
int sl2_set_graph_mode(sl2_engine* e, int enabled);
/* Which search kernel sl2_make_measurements / sl2_go_one_step use: 1 = int8 matrix-core walk (k_search_mfma, default),
 * 0 = the exact kernel with one candidate per lane (k_search_exact, the cross-check).  Identical results, bit for bit. */
int sl2_set_search_variant(sl2_engine* e, int variant);
/* Small maps (the reference's own workload: data/SceneLib2.cfg:60-62 keeps a dozen features and measures ten per frame):
 * when the whole state fits 128 columns (max_features <= 35 with one partially initialised feature) and at most 16 features
 * are measured per frame, sl2_go_one_step issues THREE launches instead of ten - predict + measurement prediction + selection,
 * the patch search, scoring + EKF update + normalise / delete / symmetrise (monoslam.cpp:108-180 unchanged in meaning;
 * search results, selection and every counter identical bit for bit, state and covariance equal to rounding).
 * The choice follows the LIVE maps, not the capacity: the engine keeps an upper bound on the number of feature slots in use
 * (exact wherever a call synchronises anyway, from a device-to-host mailbox in between; never a synchronisation of its own)
 * and takes the fused step while 13 + 3 slots + 7 <= 128 and either the batch (per sequence group) is at most 256 sequences
 * or the capacity is large (state columns >= 256: the one-stage kernels work on the whole capacity, the fused ones on the
 * live part); small capacities at large batches fuse the stages behind the search only (six launches).
 * enabled = 1 (default) / 0 = always the one-stage-per-launch kernels / 2 = fused whatever the batch size (measurements).
 * The seam entry points below always use the one-stage kernels. */
int sl2_set_step_fusion(sl2_engine* e, int enabled);
/* Search windows of at least `min_bands` bands (a band = 32 x 16 candidate positions; a window of nu x nv positions has
 * ceil(ceil(nu / 16) / 2) * ceil(nv / 16) of them) are not walked by one wavefront but cut into units of four bands that
 * extra workgroups at the end of the search launch (a quarter of it, at most 2048) work off - the window of a poorly constrained feature can be the
 * whole frame (150 bands at 320 x 240), and one wavefront walking it alone was the tail of the search.  Default: a twentieth
 * of the frame's bands (8 at 320 x 240, 96 at 1280 x 720: what is shared out should be the rare oversized window); 0 =
 * never (and no extra workgroups: they cost the headline step 0.06 %).  Results are identical either way: the parts' best
 * and second-best candidates are combined into the decision a single wavefront takes.  (An addition within SL2_API_VERSION 4 at the time: no existing entry point
 * changed; sl2_get_step_work has a 13th value.) */
int sl2_set_search_split(sl2_engine* e, int min_bands);
/* Kernel choice inside sl2_kalman_filter_update (identical algebra, results equal to rounding):
 * chol_variant 1 = one-launch left-looking Cholesky (k_chol_left; default), 0 = three launches per block column;
 * fwd_variant  1 = forward substitution with L streamed through LDS and the solved rows in registers (k_fwdsub_lds;
 *              default), 0 = operands re-read from memory (k_fwdsub).
 * Only the defaults (1, 1) are compiled into this library; the alternatives live in the TEST build
 * (libscenelib2_amd_test.so, include/scenelib2_amd_testing.h), where this call selects them - here anything else
 * returns SL2_ERR_INVALID.  (chol_variant 2, the right-looking one-launch kernel of rounds 1-2, was retired in round 6 and is
 * SL2_ERR_INVALID everywhere.)  Systems of more than 16 blocks are factored panel-wise (k_chol_left + k_fwdsub_lds +
 * k_chol_syrk per 256 columns) and systems of more than 13 blocks substituted in groups of eight block rows (k_fwd_gemm +
 * k_fwdsub_lds) either way. */
int sl2_set_update_variant(sl2_engine* e, int chol_variant, int fwd_variant);
int sl2_kalman_filter_predict(sl2_engine* e);
int sl2_auto_select_n_features(sl2_engine* e, int n);
/* Consumes the selection of the sl2_auto_select_n_features call before it (as make_measurements consumes
 * selected_feature_list_, monoslam.cpp:336-352): ONE call per selection - the list of large search windows that the selection
 * left for the search (sl2_set_search_split) is worked off and cleared by this call. */
int sl2_make_measurements(sl2_engine* e, const uint8_t* frames, size_t seq_stride, int frames_on_device);
int sl2_kalman_filter_update(sl2_engine* e);
int sl2_finish_step(sl2_engine* e, int save_trajectory);

/* MonoSLAM::elliptical_search (monoslam.cpp:401-477) as a stateless batch: `count`
 * independent searches.  image_index[i] selects one of `nimages` images (all
 * width x height).  patches [count][121]; centre [count][2]; puinv [count][3] =
 * (PuInv(0,0), PuInv(0,1), PuInv(1,1)).  Outputs: ok[count] (the bool return),
 * uv[count][2] (left untouched where no candidate qualified, Q4), score[count]
 * (corrmax).  All pointers are HOST pointers; variant 1 = production search core (int8 matrix-core walk, the one
 * k_search_mfma runs), variant 0 = the exact kernel kept for cross-checking (identical results); anything else is
 * SL2_ERR_INVALID. */
int sl2_elliptical_search_batch(int device, const uint8_t* images, int nimages, int width, int height,
                                const int32_t* image_index, const uint8_t* patches, const double* centre,
                                const double* puinv, int count, int32_t* ok, int32_t* uv, double* score,
                                int variant);

/* ----------------------------------------------------- feature initialisation */

/* MonoSLAM::find_best_patch_inside_region (monoslam.cpp:1070-1192) + find_eigenvalues (:1194-1205) as a
 * stateless batch: the Shi-Tomasi detector over `njobs` regions.  region [njobs][4] = (ustart, vstart,
 * ufinish, vfinish), clamped inside like the reference (6 px from every border for the 11x11 box);
 * uv [njobs][2] = (*ubest, *vbest) IN/OUT: left untouched when no position has a positive smaller
 * eigenvalue (evbest = 0), set to the clamped (ustart, vstart) for an empty region; evbest [njobs] = the
 * smaller eigenvalue of the winner (first maximum in scan order v outer / u inner).  Bit-exact with the
 * reference's FP64 arithmetic.  All pointers are HOST pointers; kernel_ms (optional) receives the device
 * time of the kernels alone (HIP events). */
int sl2_find_best_patch_batch(int device, const uint8_t* images, int nimages, int width, int height, int njobs,
                              const int32_t* image_index, const int32_t* region, int32_t* uv, double* evbest,
                              double* kernel_ms);

/* SearchMultipleOverlappingEllipses (improc/search_multiple_overlapping_ellipses.{h,cpp}) as a stateless
 * batch: job j = one (image, 11x11 patch) with ellipse_count[j] ellipses (the particles of one partially
 * initialised feature); ellipses of all jobs are concatenated in puinv [total][3] = (PuInv(0,0), PuInv(0,1),
 * PuInv(1,1)) and centre [total][2] (add_ellipse order).  result [total][3] = (result_flag_, result_u_,
 * result_v_); corrmax [total] (optional) = the best score of each ellipse (diagnostic).  Semantics kept:
 * centre truncated without rounding (cpp:127-128), +5.0 penalty for image sigma < 10 instead of a
 * rejection (cpp:173-175), no patch-sigma test, "<=" => last minimum in scan order wins, flag = score <= 0.40.
 * Each position of the union is scored once (the reference's cache), by the first ellipse that visits it. */
int sl2_search_multiple_overlapping_ellipses_batch(int device, const uint8_t* images, int nimages, int width, int height,
                                                   int njobs, const int32_t* image_index, const uint8_t* patches,
                                                   const int32_t* ellipse_count, const double* puinv, const double* centre,
                                                   int32_t* result, double* corrmax, double* kernel_ms);

/* ------------------------------------------------------------- frame ingest */

/* FileGrabber::ProcessFiles (framegrabber/filegrabber.cpp:63-83): every regular file below `dir`, recursively,
 * sorted by full path.  buf receives the paths separated by '\n' (may be NULL to query *count only).  Host only. */
int sl2_list_frames(const char* dir, char* buf, size_t capacity, int* count);
/* One binary PGM (P5, maxval <= 255) -> 8-bit grey, row-major, step == width (the frame contract of GoOneStep;
 * the reference decodes with cv::imread(path, 0), filegrabber.cpp:105-108).  out may be NULL to query the size.  Host only. */
int sl2_read_pgm(const char* path, uint8_t* out, size_t capacity, int* width, int* height);
/* FileGrabber::GetImageFile (filegrabber.cpp:106-109: cv::imread(path, 0)) for the three containers this library decodes,
 * chosen by the file's magic bytes: binary PGM as above; PNG (plain or Adam7-interlaced; 8-bit grey / grey+alpha / RGB / RGBA /
 * palette, 1-2-4-bit grey / palette) - grey PNGs are byte-exact, colour is reduced like libpng's rgb_to_gray, which is what
 * imread(.., 0) uses: (9797 R + 19234 G + 3737 B + 16384) >> 15; JPEG (sequential and progressive DCT, Huffman, 8 bits, one or
 * three components) - the luminance component through libjpeg's integer inverse DCT (jpeg_idct_islow), which is what
 * imread(.., 0) gets from libjpeg with out_color_space = JCS_GRAYSCALE; arithmetic-coded / lossless / 12-bit / four-component
 * files are refused with an error.  out may be NULL to query the size.  Host only. */
int sl2_read_image(const char* path, uint8_t* out, size_t capacity, int* width, int* height);
/* FileGrabber + FrameGrabber for a batch: dirs[s] is the frame directory of sequence s.  A producer thread decodes
 * (sl2_read_image: PGM, PNG or JPEG) ahead into `depth` (2..50, framegrabber.cpp:93-104) pinned host batches; sl2_ingest_next hands out
 * the next frame of every sequence in one of two device buffers for sl2_go_one_step(frames_on_device = 1).  The returned pointer
 * stays valid until the next-but-one call.
 * The upload runs on a copy stream of the grabber's own, ONE FRAME AHEAD: the call that hands out frame k also starts the copy of
 * frame k + 1 (if it is decoded), which then runs under the caller's work on frame k.
 * Stream contract: `stream` is the stream on which the caller CONSUMES the frames (the one the engine steps on: the stream given to
 * sl2_create, or sl2_get_stream of an engine-owned one).  The call makes that stream wait for frame k's copy, and takes the point
 * that stream has reached as the moment the buffer of frame k - 1 may be overwritten - so the consumer of a frame must be queued
 * on that stream BEFORE the next call.  NULL = the legacy default stream, which is ordered with every blocking stream (correct
 * with an engine-owned stream, at the price of the default stream's implicit synchronisations).
 * A decode failure is reported by the call whose frame could not be produced, not by earlier ones.
 * SL2_ERR_CAPACITY = the shortest sequence is exhausted (sl2_ingest_frame_count). */
typedef struct sl2_ingest sl2_ingest;
int sl2_ingest_open(const char* const* dirs, int nseq, int width, int height, int device, int depth, sl2_ingest** out);
int sl2_ingest_frame_count(const sl2_ingest* g);
int sl2_ingest_next(sl2_ingest* g, void* stream, const uint8_t** d_frames, size_t* seq_stride);
/* Batches of at most max_batch_bytes (nseq * width * height; default 512 KB, 0 = never) are not uploaded at all: sl2_ingest_next
 * hands out the pinned host batch itself, which the device reads in place (depth >= 4; the same stream contract - the batch goes
 * back to the decoder once the caller's stream is past the point it had reached at the NEXT call).  A single 320 x 240 sequence
 * saves the ~10 us per frame that queueing a copy costs the host.  Before the first sl2_ingest_next only. */
int sl2_ingest_set_zero_copy(sl2_ingest* g, size_t max_batch_bytes);
/* Sequences of unequal length (opt-in; sl2_ingest_next and sl2_ingest_frame_count keep their meaning).
 * sl2_ingest_frame_counts: counts[s] = frames in dirs[s], for the first min(capacity, nseq) sequences; returns nseq (< 0: bad
 * argument).
 * sl2_ingest_next_ragged: like sl2_ingest_next, but goes on until the LONGEST sequence is exhausted: call k hands out frame k
 * of every sequence that still has one and sets have[s] = 1 for those, 0 for the others (have: host [nseq]).  The part of the
 * batch that belongs to a sequence with have[s] == 0 is unspecified - nothing is decoded into it - so step with
 * sl2_set_active_sequences(e, 0, nseq, have, 0) in front of sl2_go_one_step.  Same stream contract, one-frame-ahead upload
 * and zero-copy rule as sl2_ingest_next.  SL2_ERR_CAPACITY = every sequence is exhausted.  A grabber serves ONE of the two
 * calls: the other one returns SL2_ERR_INVALID once the first has been used. */
int sl2_ingest_frame_counts(const sl2_ingest* g, int32_t* counts, int capacity);
int sl2_ingest_next_ragged(sl2_ingest* g, void* stream, const uint8_t** d_frames, size_t* seq_stride, uint8_t* have);
void sl2_ingest_close(sl2_ingest* g);

/* ------------------------------------------------------------- raw camera frames (live cameras) */

/* UsbCamGrabber::operator() (framegrabber/usbcamgrabber.cpp:75-113) for a batch: whatever the cameras deliver - RGB24 / BGR24 or
 * packed 4:2:2, any resolution, any row pitch - is reduced to 8-bit grey (cv::cvtColor) and brought to the engine's image size
 * (cv::resize, INTER_LINEAR), for every sequence in ONE launch on the device, in front of sl2_go_one_step.  The step itself keeps
 * the one image size of sl2_create; the sequences' SOURCES may all differ.
 * The arithmetic is OpenCV's 8-bit integer form of the reference's era, defined here (scenelib2_amd/csrc/sl2_convert_dev.hpp):
 *   grey   GRAY8 the byte; RGB24 / BGR24 (4899 R + 9617 G + 1868 B + 8192) >> 14; UYVY (U Y0 V Y1: the reference's
 *          CV_YUV2GRAY_Y422) row[2 x + 1]; YUYV (Y0 U Y1 V) row[2 x].  (The colour PNG path of sl2_read_image keeps libpng's
 *          constants: that is imread(.., 0), another call of the reference.)
 *   taps   along an axis of S source and D output pixels, for output d: scale = (double)S / D; f = (float)((d + 0.5) * scale - 0.5);
 *          i = floorf(f); f -= i (float); i < 0: i = 0, f = 0; i >= S - 1: i = S - 1, f = 0; i1 = min(i + 1, S - 1);
 *          w1 = rintf(f * 2048); w0 = rintf((1 - f) * 2048) (round half to even).
 *   pixel  with the column taps (x0, x1, a0, a1) and the row taps (y0, y1, b0, b1), in 32-bit integers: H(y) = g[y][x0] a0 + g[y][x1] a1;
 *          out = (((b0 (H(y0) >> 4)) >> 16) + ((b1 (H(y1) >> 4)) >> 16) + 2) >> 2.
 * It is the identity where source and output size agree and maps a constant image to itself.  The taps are evaluated on the host
 * and uploaded as tables: the kernel and sl2_convert_frame_host do integer work on the same tables and agree byte for byte.
 *
 * Machine-vision cameras (GenICam / USB3 Vision / GigE: Mono10 / Mono12 / Mono16, BayerRG8 and its siblings) deliver deep grey or a
 * raw Bayer mosaic.  Their grey g[y][x] is defined here - no OpenCV exists to compare with: parity with OpenCV unpinned - and both
 * resize filters then act on it exactly as on the grey of the five formats above:
 *   deep grey, N = 10, 12, 16   16-bit little-endian words: v = row[2 x] | row[2 x + 1] << 8; g = (v & (2^N - 1)) >> (N - 8): the top
 *          eight significant bits, truncated; bits above N are ignored.  offset and pitch are even, and so is the address of a raw
 *          buffer that is on the device.  (Big-endian 16-bit needs no format: truncated to its top byte it is a SL2_PIX_YUYV source.)
 *   Bayer  one byte a pixel, p[y][x]; the format's name is the 2 x 2 tile at the SOURCE's pixel (0,0), top row then bottom row, so
 *          the colour of site (x, y) is letter (y & 1) * 2 + (x & 1) of the name, and a region of interest that starts on an odd
 *          sensor column or row is the matching sibling.  Indices are reflected about the edge pixel (-1 -> 1, S -> S - 2), which
 *          keeps the colour phase; width and height are at least 2, odd sizes allowed.  With c = p[y][x], h2 = left + right,
 *          v2 = up + down, cross4 = h2 + v2 and diag4 = the four diagonals, (R4, G4, B4) is
 *            at a red site (4 c, cross4, diag4), at a blue site (diag4, cross4, 4 c),
 *            at a green site with red to its left and right (2 h2, 4 c, 2 v2), with blue to its left and right (2 v2, 4 c, 2 h2),
 *          and g = (4899 R4 + 9617 G4 + 1868 B4 + 32768) >> 16: bilinear demosaic in exact quarters, then the grey weights above,
 *          one rounding (at most 16384 * 1020 + 32768: 32 bits).  A constant mosaic maps to itself; a mosaic sampled from a flat
 *          colour (R, G, B) gives the RGB24 grey of (R, G, B) at every pixel.
 * Not covered: Bayer in 10, 12 or 16-bit containers, packed 10 or 12-bit (Mono12p), edge-aware demosaic, white balance, gamma. */
enum { SL2_PIX_GRAY8 = 0, SL2_PIX_RGB24 = 1, SL2_PIX_BGR24 = 2, SL2_PIX_UYVY = 3, SL2_PIX_YUYV = 4,      /* 5 .. 15: unassigned */
       SL2_PIX_GRAY10 = 16, SL2_PIX_GRAY12 = 17, SL2_PIX_GRAY16 = 18,      /* 16-bit little-endian words, the low N bits significant */
       SL2_PIX_BAYER_RGGB8 = 24, SL2_PIX_BAYER_GRBG8 = 25, SL2_PIX_BAYER_GBRG8 = 26, SL2_PIX_BAYER_BGGR8 = 27 };
typedef struct sl2_frame_source {        /* 24 bytes */
  int32_t width, height;                 /* source pixels: 1 .. 4096 by 1 .. 16384; even width for the 4:2:2 formats; 2 at least for Bayer */
  int32_t pitch;                         /* bytes from one source row to the next, >= the row's own bytes; even for the 16-bit formats */
  int32_t format;                        /* SL2_PIX_* */
  uint64_t offset;                       /* of this sequence's first byte inside the raw buffer */
} sl2_frame_source;
typedef struct sl2_converter sl2_converter;
/* A converter for nseq sequences to out_width x out_height (1 .. 4096 each; the engine's image size).  It needs no engine. */
int sl2_converter_create(int device, int nseq, int out_width, int out_height, sl2_converter** out);
void sl2_converter_destroy(sl2_converter* c);
/* The sources of sequences seq0 .. seq0 + nseq - 1.  A setup call: it may wait (for the last conversion queued, which keeps the
 * tables it was queued with) and takes effect for the sl2_convert_frames calls after it.  Two sequences may name the same bytes
 * (one camera feeding two filters).  Refused (SL2_ERR_INVALID, nothing changed, the text names the sequence): width or height
 * below 1 or over the cap, pitch below the bytes of a row, an odd width with a 4:2:2 format, an unknown format, a Bayer source
 * under 2 pixels on an axis, an odd offset or pitch with a 16-bit format.
 * sl2_converter_get_sources returns what was set (SL2_ERR_INVALID for a sequence never set). */
int sl2_converter_set_sources(sl2_converter* c, int seq0, int nseq, const sl2_frame_source* src);
int sl2_converter_get_sources(const sl2_converter* c, int seq0, int nseq, sl2_frame_source* src);
/* Converts every sequence: d_frames[s * seq_stride + y * out_width + x], a device buffer of the caller's (sl2_dev_malloc); the
 * bytes between out_width * out_height and seq_stride are left untouched.  Asynchronous on `stream` (a hipStream_t; the stream
 * the engine steps on): sl2_go_one_step(.., frames_on_device = 1) queued after it on that stream needs no other ordering.
 * raw_on_device = 0: raw is host memory; its raw_bytes are first copied, on `stream`, to a staging buffer of the converter's
 * own, which grows on demand (never in the steady state).  The host buffer may be reused once `stream` has passed the copy
 * (after sl2_synchronize, say); pageable memory has been read when the call returns, pinned memory has not.
 * Refused on the host, before anything is queued (SL2_ERR_INVALID, the text names the sequence): a sequence whose source was
 * never set, a source that reaches past the buffer (offset + (height - 1) * pitch + the bytes of a row > raw_bytes),
 * seq_stride < out_width * out_height. */
int sl2_convert_frames(sl2_converter* c, void* stream, const void* raw, size_t raw_bytes, int raw_on_device,
                       uint8_t* d_frames, size_t seq_stride);
/* The same arithmetic for one sequence on the host (no GPU needed): out[out_height][out_width].  Same refusals. */
int sl2_convert_frame_host(const sl2_frame_source* src, const void* raw, size_t raw_bytes, int out_width, int out_height,
                           uint8_t* out);
/* The resize filter, per sequence.  SL2_RESIZE_LINEAR (the default) is the two-tap form above: right for the reference's 640 x 480
 * webcam, but it reads two source rows and two source columns per output pixel whatever the reduction, and what lies between them
 * aliases.  SL2_RESIZE_AREA is the exact box average: every source pixel under an output pixel, weighted by the area they share.
 * Integers only, no tables (scenelib2_amd/csrc/sl2_convert_dev.hpp):
 *   grey    g[y][x] as above, all formats.
 *   weights along an axis of S source and D output pixels, S >= D, in units of 1/D of a source pixel: output d covers
 *           [d S, (d + 1) S), source i covers [i D, (i + 1) D).  The taps of d are i = floor(d S / D) .. floor(((d + 1) S - 1) / D) and
 *           w(d, i) = min((i + 1) D, (d + 1) S) - max(i D, d S): 1 .. D each, summing to S over one output and to D over one source.
 *   pixel   acc = sum_y sum_x wy(dy, y) wx(dx, x) g[y][x], exact (at most 255 Sx Sy < 2^34 at the caps);
 *           out = floor((2 acc + Sx Sy) / (2 Sx Sy)): the exact mean, halves rounded up.
 * It is the identity where source and output size agree and maps a constant image to itself.  It only reduces: a source narrower
 * or lower than the output is refused under SL2_RESIZE_AREA (no per-axis fallback).
 * Planar and semi-planar 4:2:0 frames (NV12, NV21, I420, YV12) need no format of their own: their luma plane is a SL2_PIX_GRAY8
 * source of `height` rows with the plane's pitch, and the chroma that follows is never reached.
 * sl2_converter_set_filters: a setup call like sl2_converter_set_sources (it may wait for the last conversion queued, which keeps
 * the filters it was queued with), before or after the sequence's source is set.  Refused (SL2_ERR_INVALID, no sequence of the
 * range changes, the text names the sequence): a filter id other than these two; SL2_RESIZE_AREA for a sequence whose source is
 * set and is smaller than the output on an axis.  sl2_converter_set_sources refuses such a source for a sequence whose filter is
 * SL2_RESIZE_AREA.  sl2_converter_get_filters works for any sequence, its source set or not.
 * sl2_convert_frames then issues one more launch (k_convert_area) for the SL2_RESIZE_AREA sequences; with none it is unchanged.
 * Deep grey and Bayer sequences likewise have a launch of their own per filter (k_raw_linear, k_raw_area): four launches at most.
 * sl2_convert_frame_host_filtered: the host form; with SL2_RESIZE_LINEAR the bytes of sl2_convert_frame_host.  Its refusals, plus
 * an unknown filter and a source smaller than the output under SL2_RESIZE_AREA. */
enum { SL2_RESIZE_LINEAR = 0, SL2_RESIZE_AREA = 1 };
int sl2_converter_set_filters(sl2_converter* c, int seq0, int nseq, const int32_t* filters);
int sl2_converter_get_filters(const sl2_converter* c, int seq0, int nseq, int32_t* filters);
int sl2_convert_frame_host_filtered(const sl2_frame_source* src, int filter, const void* raw, size_t raw_bytes,
                                    int out_width, int out_height, uint8_t* out);
/* The calibration of the resized image from that of the source image (in->width, in->height = the source size): with
 * s = in->width / out_width, fku' = fku / s, fkv' = fkv / s, u0' = (u0 + 0.5) / s - 0.5, v0' likewise, kd1' = kd1 s s; sd is
 * unchanged (the measurement noise in output pixels is the caller's choice).  The radial term lives in centred pixels and
 * survives a uniform scale only: in->width * out_height != in->height * out_width is refused (SL2_ERR_INVALID) - the
 * conversion itself accepts any aspect ratio.  Host only. */
int sl2_scale_camera(const sl2_camera* in, int out_width, int out_height, sl2_camera* out);

/* ---- the lens remap (additions within SL2_API_VERSION 5): a sequence follows a per-pixel map instead of a resize filter ----
 * The filter knows one lens model, the reference's single-coefficient radial one (sl2_camera.kd1; Camera::Project / Unproject,
 * camera.cpp:90-154).  Calibrations come as OpenCV's k1 k2 p1 p2 k3 [k4 k5 k6] or its fisheye k1 .. k4.  A map brings such a
 * camera's frames into an image the filter's model describes: cv::initUndistortRectifyMap plus cv::remap, for the whole batch in
 * one launch in front of the step.  The map is the general primitive: a rotated or mirrored mount, a crop, a stereo
 * rectification or a lens model of the caller's own are maps too (sl2_lens_map_host below builds the ones from calibrations).
 *
 * A map belongs to a source size W x H and to the converter's output size: int32_t xy[out_height][out_width][2].  (X, Y) is the
 * position in the source's grey plane in 1/32 of a source pixel; pixel centres sit on integers, X = 32 x is column x (the
 * convention of sl2_rectify_frames); X == SL2_REMAP_BORDER means no source (Y is then ignored).  Per output pixel, in 32-bit integers
 * (scenelib2_amd/csrc/sl2_convert_dev.hpp, remap_pixel):
 *   a border entry gives 0.  Otherwise fx = X & 31, ix = (X - fx) / 32, fy = Y & 31, iy = (Y - fy) / 32 (two's complement: fx, fy
 *   in 0 .. 31 and ix, iy the floors, for negative positions too);
 *   a tap p(ix, iy) is g[iy][ix] where 0 <= ix < W and 0 <= iy < H, else 0; g is the grey defined above for the source's format -
 *   for Bayer the demosaic, with its own reflection for the neighbours of an in-image tap; a neighbour whose weight is 0 is not read
 *   (it needs no source pixel: X = 32 (W - 1) is the last column itself; both forms fetch the byte of a tap that does not count
 *   from the clamped, in-image coordinate and discard it, so nothing outside the W x H source is ever addressed);
 *   out = ((32 - fx)(32 - fy) p(ix, iy) + fx (32 - fy) p(ix + 1, iy) + (32 - fx) fy p(ix, iy + 1) + fx fy p(ix + 1, iy + 1) + 512) >> 10.
 * It is the identity for the identity map (X = 32 x, Y = 32 y at equal sizes) and maps a constant source to the same constant
 * wherever all four taps lie inside.  It applies NO anti-aliasing: two taps an axis whatever the map's local scale, so a map that
 * reduces by much more than two aliases like SL2_RESIZE_LINEAR (reduce with a larger output, or remap a source the camera bins).
 *
 * sl2_converter_set_map: the converter has nseq map slots, 0 .. nseq - 1, empty after create.  The call fills or replaces one
 * slot with a map for sources of src_width x src_height; xy is consumed before it returns; xy == NULL empties the slot.  A setup
 * call like sl2_converter_set_sources: it may wait for the last conversion queued, which keeps the map it was queued with.  An
 * entry that can reach no source pixel with a weight above 0 is kept as the border entry (the result is 0 either way).
 * Refused (SL2_ERR_INVALID, nothing changed): a slot outside the range; a size outside the source caps (1 .. 4096 by 1 .. 16384);
 * emptying a slot, or changing the size of one, that a sequence still uses (the text names the first such sequence).
 * sl2_converter_set_remaps / sl2_converter_get_remaps: the slot of each sequence of seq0 .. seq0 + nseq - 1, or -1 for none (the
 * state after create).  Many sequences may share a slot: a fleet of identical cameras.  A sequence with a map ignores its resize
 * filter; the filter stays set (and stays checked against the source) and acts again once the slot is -1.  Refused (SL2_ERR_INVALID, no
 * sequence of the range changes, the text names the sequence): a slot outside -1 .. nseq - 1, an empty slot, a sequence whose
 * source is set with another size than the map's.  sl2_converter_set_sources likewise refuses a source whose size differs from
 * its sequence's map.
 * sl2_convert_frames then issues one more launch (k_convert_remap) for the mapped sequences, which leave the other kernels'
 * lists; with no mapped sequence nothing new is launched and no existing launch changes.
 * sl2_remap_frame_host: the host form for one sequence (no GPU needed); the map is one for src->width x src->height.  The
 * refusals of sl2_convert_frame_host, and xy == NULL.
 * Not covered: an anti-aliased remap; maps on the device (a map is set from host memory). */
#define SL2_REMAP_BORDER INT32_MIN
int sl2_converter_set_map(sl2_converter* c, int slot, int src_width, int src_height, const int32_t* xy);
int sl2_converter_set_remaps(sl2_converter* c, int seq0, int nseq, const int32_t* slots);
int sl2_converter_get_remaps(const sl2_converter* c, int seq0, int nseq, int32_t* slots);
int sl2_remap_frame_host(const sl2_frame_source* src, const int32_t* xy, const void* raw, size_t raw_bytes, int out_width,
                         int out_height, uint8_t* out);

/* ---- maps from calibrations (additions within SL2_API_VERSION 5; host only, no device) ----
 * sl2_lens_map_host fills xy[target->height][target->width][2] with the map that takes an image `target` would have seen and
 * reads it out of the lens's image (lens->width x lens->height, the map's source size).  `target` is the calibration the engine
 * will run with (sl2_create / sl2_set_cameras); its width and height are the converter's output size.  Any target is accepted.
 * FP64, no contraction into fused multiply-adds, every line in the order written, parentheses included.  For target pixel (x, y):
 *   cx = x - u0;  cy = y - v0;  f = 1 - (2 kd1) (cx cx + cy cy);  if f > 0 does not hold the entry is the border;
 *   s = sqrt(f);  a = (cx / s) / fku;  b = (cy / s) / fkv.
 * (a, b) are image-plane coordinates, x to the right and y down: OpenCV's x', y'.  The reference's camera axes point the other way
 * (u = u0 - fku X / Z), but both conventions put u at u0 + fku x', so the image is neither mirrored nor turned.
 * With (fx, fy, cx, cy) and k[] now the LENS's, the source position (us, vs) is
 *   SL2_LENS_RADIAL1 (the reference's own model, k[0] = kd1):  px = fx a;  py = fy b;  q = 1 + (2 k[0]) (px px + py py);
 *     if q > 0 does not hold the entry is the border;  s = sqrt(q);  us = px / s + cx;  vs = py / s + cy.
 *   SL2_LENS_BROWN (OpenCV's order: k[0..7] = k1 k2 p1 p2 k3 k4 k5 k6):  r2 = a a + b b;  r4 = r2 r2;  r6 = r4 r2;
 *     num = ((1 + k1 r2) + k2 r4) + k3 r6;  den = ((1 + k4 r2) + k5 r4) + k6 r6;  den == 0 is the border;  rad = num / den;  ab = a b;
 *     xd = (a rad + (2 p1) ab) + p2 (r2 + 2 (a a));  yd = (b rad + p1 (r2 + 2 (b b))) + (2 p2) ab;  us = fx xd + cx;  vs = fy yd + cy.
 *   SL2_LENS_FISHEYE (Kannala-Brandt as OpenCV's fisheye, k[0..3] = k1 .. k4):  r = sqrt(a a + b b);  r == 0 gives (cx, cy);  else
 *     th = atan(r);  t2 = th th;  t4 = t2 t2;  t6 = t4 t2;  t8 = t4 t4;  thd = th ((((1 + k1 t2) + k2 t4) + k3 t6) + k4 t8);
 *     sc = thd / r;  us = fx (a sc) + cx;  vs = fy (b sc) + cy.
 * A position that is not finite or lies beyond +-2^20 is the border.  Otherwise X = floor(us 32 + 0.5), Y = floor(vs 32 + 0.5).
 * Only atan is not correctly rounded everywhere: a FISHEYE entry may differ by one unit between two C libraries where
 * us 32 + 0.5 lies within an ulp or so of an integer; RADIAL1 and BROWN are exact (+ - x / sqrt).
 * What the target costs: sl2_lens_pinhole_camera (kd1 = 0) is the obvious one, but a wide lens keeps its field better under a
 * target with kd1 > 0 - a pinhole target of the same focal length stretches the periphery, one of a shorter focal length gives
 * the centre fewer pixels.  Where the map leaves the lens's image the output is the border (0), which the filter sees as texture.
 * Refused (SL2_ERR_INVALID): a NULL, an unknown model, a lens size outside the source caps, a target size outside 1 .. 4096.
 * Not covered: a polynomial that folds back beyond the calibrated field maps far target pixels onto near source pixels (the
 * caller's problem: OpenCV does not guard it either); parity with OpenCV itself is unpinned - none exists where this was
 * written; this text is the definition.
 * sl2_lens_pinhole_camera: the pinhole target that sees the lens's image plane resized to out_width x out_height: kd1 = 0,
 * fku = fx out_width / width, fkv = fy out_height / height (the product first), u0 = (cx + 0.5) out_width / width - 0.5, v0
 * likewise with the heights; sd as given.  With a zero-distortion lens the map is then the plain resize's. */
enum { SL2_LENS_RADIAL1 = 0, SL2_LENS_BROWN = 1, SL2_LENS_FISHEYE = 2 };
typedef struct sl2_lens {                /* 112 bytes */
  int32_t model, width, height;          /* SL2_LENS_*; the size of the lens's image: the map's source size */
  double fx, fy, cx, cy;                 /* pixels, OpenCV's camera matrix (pixel centres on integers) */
  double k[8];                           /* by model, see above; the rest ignored */
} sl2_lens;
int sl2_lens_map_host(const sl2_lens* lens, const sl2_camera* target, int32_t* xy);
int sl2_lens_pinhole_camera(const sl2_lens* lens, int out_width, int out_height, int sd, sl2_camera* out);

/* ---- the frame monitor (additions within SL2_API_VERSION 5): per-sequence frame statistics and a device-side gate ----
 * Nothing else looks at a frame before the step.  A monitor is an object beside the engine, like the converter: in two
 * stream-ordered launches it examines the engine-size grey frames of a whole batch, writes an exact integer record per sequence,
 * compares it with the sequence's thresholds and writes a verdict word and an `active` byte per sequence - bytes that
 * sl2_set_active_sequences(.., on_device = 1) takes as they are, so a camera that repeated its buffer or delivered a black frame
 * sits the step out without a host round trip.  Every rule is off by default; an engine without a monitor launches nothing new.
 *
 * A frame is n = width * height bytes f[0 .. n), row-major with pitch = width (the engine's own frame format).  The record:
 *   sum, sum_sq      of f[i] and of f[i]^2.
 *   gradient_energy  sum over 1 <= x <= W - 2, 1 <= y <= H - 2 of (f[y][x+1] - f[y][x-1])^2 + (f[y+1][x] - f[y-1][x])^2; 0 when W < 3 or
 *                    H < 3.
 *   digest           positional, and a sum, so the order of accumulation does not matter.  Word k, 0 <= k < ceil(n / 8), is the
 *                    sum over j < 8 with 8 k + j < n of (uint64) f[8 k + j] << 8 j; digest = sum over k of
 *                    mix64(word_k ^ ((k + 1) * 0x9E3779B97F4A7C15)) mod 2^64, where mix64(z) is
 *                      z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31.
 *                    The word index is relative to the frame: not to the pointer's alignment, not to seq_stride.
 *   min, max         of f[i].
 *   hist[16]         hist[f[i] >> 4].
 * The host form and the kernels meet this text bit for bit (one source: scenelib2_amd/csrc/sl2_frame_monitor_dev.hpp).
 * The gate of a sequence: every comparison is on integers, the verdict is the OR of the rules that fire, 0 = the frame passes.
 * Not covered: a difference against the previous frame's PIXELS (a noisy camera that repeats a scene is not REPEATED: the digest
 * changes with one byte); raw-format frames in front of the converter; statistics per region.  The monitor's state (gates,
 * previous digests) belongs to the monitor and is in no sequence blob, as the mask belongs to the engine. */
typedef struct sl2_frame_stats {         /* 104 bytes */
  uint64_t sum;
  uint64_t sum_sq;
  uint64_t gradient_energy;
  uint64_t digest;
  uint32_t min, max;
  uint32_t hist[16];
} sl2_frame_stats;
typedef struct sl2_frame_gate {          /* 32 bytes; all zeros = every rule off */
  uint32_t min_range;                    /* SL2_FRAME_FLAT     when max - min < min_range (0: off) */
  uint32_t dark_bins;                    /* bins [0, dark_bins) are dark, 0 .. 16 (0: off) */
  uint32_t max_dark_pixels;              /* SL2_FRAME_DARK     when more dark pixels than this */
  uint32_t bright_bins;                  /* bins [16 - bright_bins, 16) are bright, 0 .. 16 (0: off) */
  uint32_t max_bright_pixels;            /* SL2_FRAME_BRIGHT   when more bright pixels than this */
  uint32_t reject_repeated;              /* SL2_FRAME_REPEATED when digest == digest of the sequence's previous EXAMINED frame (0: off) */
  uint64_t min_gradient_energy;          /* SL2_FRAME_BLURRED  when gradient_energy < this (0: off) */
} sl2_frame_gate;
enum { SL2_FRAME_FLAT = 1, SL2_FRAME_DARK = 2, SL2_FRAME_BRIGHT = 4, SL2_FRAME_BLURRED = 8, SL2_FRAME_REPEATED = 16, SL2_FRAME_SKIPPED = 32 };
typedef struct sl2_frame_monitor sl2_frame_monitor;
/* A monitor for `batch` sequences of width x height frames: width, height >= 1 and width * height < 2^31.  It needs no engine.
 * After creation every gate is all zeros and no sequence has a previous digest. */
int sl2_frame_monitor_create(int device, int batch, int width, int height, sl2_frame_monitor** out);
void sl2_frame_monitor_destroy(sl2_frame_monitor* m);
/* The gates of sequences seq0 .. seq0 + nseq - 1: host memory, consumed before the call returns; the change is ordered on the
 * stream of the next examination (it rides in front of it, as one small launch per 64 consecutive sequences whose gate was set
 * since the last examination; an examination with no gate set since then is the two launches alone) and the call never waits.  SL2_ERR_INVALID, and nothing changed: a
 * NULL, a range outside the batch, dark_bins > 16 or bright_bins > 16 in any gate of the range (the text names the sequence).
 * sl2_frame_monitor_get_gates returns what was set. */
int sl2_frame_monitor_set_gates(sl2_frame_monitor* m, int seq0, int nseq, const sl2_frame_gate* gates);
int sl2_frame_monitor_get_gates(const sl2_frame_monitor* m, int seq0, int nseq, sl2_frame_gate* gates);
/* Forgets the previous digests of the range (a slot given to another camera): the next examined frame of such a sequence is not
 * REPEATED.  Ordered like sl2_frame_monitor_set_gates; never waits. */
int sl2_frame_monitor_reset(sl2_frame_monitor* m, int seq0, int nseq);
/* Examines frames + b * seq_stride for every sequence b of the batch, asynchronously on `stream` (a hipStream_t): two launches,
 * k_frame_stats and k_frame_gate; the call never waits for the device.  All pointers are device pointers and every one but
 * `frames` may be NULL: base_active [batch] bytes (NULL: all ones), stats_out [batch] records, verdict_out [batch] words,
 * active_out [batch] bytes.  frames + b * seq_stride may have any alignment and seq_stride any value >= width * height; the bytes
 * between are not read.  A sequence with base_active[b] == 0 is not examined: none of its frame bytes are read, its stats_out
 * record and its previous digest are left as they were, its verdict is SL2_FRAME_SKIPPED and its active_out[b] is 0.  Otherwise
 * the verdict is the OR of the rules that fire, active_out[b] = (verdict == 0), and the sequence's previous digest becomes this
 * frame's, whatever the verdict; the first examined frame of a sequence is never REPEATED.  Every quantity is an integer sum, a
 * minimum or a maximum: the outputs are the same bytes on every run.  base_active and active_out may be the same array. */
int sl2_examine_frames(sl2_frame_monitor* m, void* stream, const uint8_t* frames, size_t seq_stride, const uint8_t* base_active,
                       sl2_frame_stats* stats_out, uint32_t* verdict_out, uint8_t* active_out);
/* The last examination of the range, to host memory: the record each sequence was last examined with (zeros before the first)
 * and the last call's verdicts (SL2_FRAME_SKIPPED before the first).  Either pointer may be NULL.  Synchronises. */
int sl2_frame_monitor_read(sl2_frame_monitor* m, int seq0, int nseq, sl2_frame_stats* stats, uint32_t* verdicts);
/* The host forms (no GPU needed).  sl2_frame_stats_host: the record of one frame; SL2_ERR_INVALID for a NULL or a size outside
 * the monitor's.  sl2_frame_verdict_host: the verdict word of a record under a gate; have_previous != 0 = the sequence has a
 * previous digest, previous_digest.  A NULL or a gate the setter would refuse gives 0xFFFFFFFF (no verdict has those bits). */
int sl2_frame_stats_host(const uint8_t* frame, int width, int height, sl2_frame_stats* stats);
uint32_t sl2_frame_verdict_host(const sl2_frame_stats* stats, const sl2_frame_gate* gate, int have_previous, uint64_t previous_digest);

/* ----------------------------------------------------------------- state access */

/* total_state_size_ per sequence (13 + 3 * live features). */
int sl2_get_total_state_sizes(sl2_engine* e, int seq0, int nseq, int32_t* sizes);
/* construct_total_state / construct_total_covariance (monoslam.cpp:501-546) for one
 * sequence, deleted features removed: x [n], P [n][n], n = total state size. */
int sl2_get_total_state(sl2_engine* e, int seq, double* x, int capacity);
int sl2_get_total_covariance(sl2_engine* e, int seq, double* P, int capacity_n);
/* feature_list_ of one sequence in list order (deleted features skipped unless
 * include_deleted).  Returns the number written through *count. */
int sl2_get_features(sl2_engine* e, int seq, sl2_feature_info* out, int capacity, int include_deleted, int* count);
/* Entry `index` of feature_init_info_vector_ of one sequence (FeatureInitInfo + its particles, feature_init_info.h:46-118;
 * up to params.max_features_to_init_at_once <= 4 entries, in the vector's order).
 * ints [16] = feature_init_info_vector_.size(), label, number_of_match_attempts_, #particles,
 * making_measurement_on_this_step_flag_, uu_, vv_, region_defined (this step), init_feature_search_{ustart,vstart,ufinish,vfinish}_,
 * #initialised, #converted, #deleted (totals for this sequence), created (this step); dbl [9] = mean_, covariance_, y_(0..5),
 * evbest of the last detection; particles [capacity][12] = lambda_, probability_, cumulative_probability_, m_h_(2), m_z_(2),
 * m_SInv_(00,01,11), m_detS_, m_successful_measurement_flag_ (may be NULL).  ints [0] and the sequence-level entries (5..15,
 * dbl [8]) are filled for any index; the feature's own entries are zero when index >= ints [0]. */
int sl2_get_partial_feature(sl2_engine* e, int seq, int index, int32_t* ints, double* dbl, double* particles, int capacity);
/* Feature::patch_ (feature.h:118; 11x11, row-major) of the feature with this label: the template given to
 * sl2_add_known_features, or the one copy_into_patch cut from the frame when the feature was initialised
 * (monoslam.cpp:1236-1250).  Labels of deleted features keep their last template. */
int sl2_get_feature_patch(sl2_engine* e, int seq, int label, uint8_t* patch121);
/* ---- one-call read-back of everything the reference exposes as public members (monoslam.h:158-218, feature.h:78-142) ----
 *
 * The reference's caller reads xv_, Pxx_, feature_list_[i]->{y_, Pxy_, Pyy_, h_, z_, S_, ...}, selected_feature_list_,
 * trajectory_store_ and feature_init_info_vector_ straight out of the object after every GoOneStep
 * (examples/MonoSlamSceneLib1.cpp:132-151, graphic/graphictool.cpp:130-167, 290-347).  sl2_snapshot is that read for one
 * sequence: ONE kernel packs the blob below on the device and streams it into an engine-owned pinned host buffer, ONE
 * stream synchronisation follows, and *blob points into that buffer (valid until the next sl2_snapshot / sl2_destroy on
 * this engine; no allocation per call).
 *
 *   traj_cursor       number of trajectory_store_ pushes the caller has already seen (0 the first time): the blob carries
 *                     the entries [max(traj_cursor, total - 1000), total) - the caller appends them and drops from the
 *                     front beyond 1000 entries like monoslam.cpp:172-177;
 *   patch_from_label  the 11 x 11 templates (Feature::patch_) of the live features whose label_ is >= this value are
 *                     included (labels are handed out once and a feature's template never changes, so a caller that caches
 *                     templates by label passes its next_free_label_ of the previous call; 0 = all, INT32_MAX = none).
 *
 * Blob layout (every section starts on an 8-byte boundary; offsets in bytes from the start of the blob):
 *   sl2_snapshot_header
 *   off_xv         double[13]                      xv_
 *   off_Pxx        double[13][13]                  Pxx_
 *   off_features   sl2_feature_info[n_features]    feature_list_ order, deleted features removed
 *   off_cov        per feature, in the same order: Pxy_ (13 x d, row-major) then Pyy_ (d x d), d = state_size (3 or 6)
 *   off_selection  int32[n_selected]               selected_feature_list_ as labels, selection order
 *   off_traj       double[traj_count][3]           trajectory_store_ entries traj_first .. traj_first + traj_count - 1
 *   off_partial    n_partial records, feature_init_info_vector_ order: sl2_partial_info, then double[n_particles][12]
 *                  (lambda_, probability_, cumulative_probability_, m_h_(2), m_z_(2), m_SInv_(00, 01, 11), m_detS_,
 *                  m_successful_measurement_flag_)
 *   off_patches    n_patches records of 128 bytes: int32 label, uint8[121] patch (row-major), 3 bytes of padding */
typedef struct sl2_snapshot_header {
  int32_t magic;                               /* 0x53324c53 ("SL2S") */
  int32_t api_version;                         /* SL2_API_VERSION of the library */
  int32_t bytes;                               /* size of the whole blob */
  int32_t seq;
  int32_t n_features;                          /* feature_list_.size() */
  int32_t total_state_size;                    /* total_state_size_ */
  int32_t number_of_visible_features;          /* number_of_visible_features_ */
  int32_t n_selected;                          /* selected_feature_list_.size() */
  int32_t successful_measurement_vector_size;  /* successful_measurement_vector_size_ */
  int32_t next_free_label;                     /* next_free_label_ */
  int32_t status_flags;                        /* SL2_STATUS_* */
  int32_t traj_total, traj_first, traj_count;
  int32_t n_partial;                           /* feature_init_info_vector_.size() */
  int32_t n_patches;
  int32_t uu, vv;                              /* uu_, vv_ */
  int32_t location_selected_flag;              /* location_selected_flag_ */
  int32_t init_feature_search_region_defined_flag;
  int32_t init_feature_search_region[4];       /* ustart, vstart, ufinish, vfinish */
  int32_t off_xv, off_Pxx, off_features, off_cov, off_selection, off_traj, off_partial, off_patches;
  int32_t steps_done;                          /* GoOneStep calls so far (low 31 bits) */
  int32_t sequence_steps;                      /* steps this SEQUENCE has taken (low 31 bits): differs from steps_done once the
                                                  sequence was loaded, copied in or reset (sl2_load_sequences below) */
  int32_t omitted_sections;                    /* SL2_SNAP_* bits of the sections this blob does not carry (sl2_snapshot: 0) */
  int32_t reserved[29];
} sl2_snapshot_header;                         /* 256 bytes */
typedef struct sl2_partial_info {              /* FeatureInitInfo, feature_init_info.h:77-118 */
  int32_t label;                               /* fp_->label_ */
  int32_t number_of_match_attempts;
  int32_t n_particles;                         /* particle_vector_.size() */
  int32_t making_measurement_on_this_step_flag;
  double mean, covariance;                     /* mean_, covariance_ of lambda */
} sl2_partial_info;                            /* 32 bytes, followed by the particles */
/* Upper bound of a blob of this engine in bytes. */
size_t sl2_snapshot_capacity(const sl2_engine* e);
int sl2_snapshot(sl2_engine* e, int seq, int traj_cursor, int patch_from_label, const void** blob, size_t* bytes);

/* ---- the same read for a RANGE of sequences in one call (additions within SL2_API_VERSION 5) ----
 *
 * sl2_snapshot serves one sequence per launch and wait; a caller that publishes every sequence of a large batch after every frame
 * pays that B times.  sl2_snapshot_batch packs the blobs of sequences seq0 .. seq0 + nseq - 1 back to back in three launches on
 * the engine's stream (sizes, their exclusive scan, one workgroup per blob), carries only the sections asked for, and either hands
 * the packed bytes to the host in one copy or leaves them in the caller's device memory without waiting at all.
 *
 *   sections  SL2_SNAP_* bits.  The header, xv_ and Pxx_ are always present (SL2_SNAP_POSE = 0 names that choice).  An omitted
 *             section has length 0 and its off_* is the running offset (off_next - off_this == 0); header.omitted_sections =
 *             SL2_SNAP_ALL & ~sections.  Counts that describe the SEQUENCE stay true whatever is omitted (n_features,
 *             total_state_size, n_selected, n_partial, traj_total, next_free_label ...); counts that describe what the BLOB
 *             carries follow the blob: without SL2_SNAP_TRAJ traj_count = 0 and traj_first = traj_total, without SL2_SNAP_PATCHES
 *             n_patches = 0.  SL2_SNAP_COV without SL2_SNAP_FEATURES is refused: the covariance records cannot be walked without
 *             each feature's state_size.
 *   cursors   [nseq][2] = (traj_cursor, patch_from_label) per sequence, with sl2_snapshot's meaning; NULL = (0, 0) for all.
 *   blobs     blob i is the sl2_snapshot blob of sequence seq0 + i restricted to `sections`; with SL2_SNAP_ALL it is byte for
 *             byte what sl2_snapshot(e, seq0 + i, cursors[i][0], cursors[i][1], ..) returns at that point of the stream.
 *   packing   offsets [nseq + 1]: offsets[0] = 0, offsets[i + 1] - offsets[i] = header.bytes of blob i rounded up to 16,
 *             offsets[nseq] = the total.  Blob i starts at out + offsets[i]; the bytes between header.bytes and the next start
 *             are zero; nothing at or beyond out + offsets[nseq] is written.
 *
 * Host form (on_device == 0): out, offsets and cursors are host memory of any kind; cursors is consumed before the call returns.
 * The blobs are packed into device staging owned by the engine (sized sl2_snapshot_bound x nseq on first use, grown on demand,
 * never in the steady state); the offset table comes back first (a small copy and the call's one wait for the device), then
 * exactly offsets[nseq] bytes in one copy.  If offsets[nseq] > out_bytes the call returns SL2_ERR_CAPACITY with offsets filled -
 * the caller learns the size it needs - and out untouched.
 * Device form (on_device != 0): out (16-byte aligned), offsets and cursors are device pointers; the call is the three launches
 * and never waits.  If the total exceeds out_bytes no blob is written (the pack kernel checks that itself); offsets is written
 * either way.  A consumer on the engine's stream needs no other ordering.
 * Both forms drop no captured step, change nothing in the engine, work with sequence groups (as sl2_snapshot) and treat a paused
 * sequence like any other.
 * Refused (SL2_ERR_INVALID, nothing queued): a null engine, out or offsets; a range outside the batch or nseq < 1; sections with
 * bits outside SL2_SNAP_ALL; SL2_SNAP_COV without SL2_SNAP_FEATURES; a device `out` that is not 16-byte aligned; host form only:
 * a negative traj_cursor (the device form cannot look: it takes a negative cursor as 0). */
enum { SL2_SNAP_POSE = 0, SL2_SNAP_FEATURES = 1, SL2_SNAP_COV = 2, SL2_SNAP_SELECTION = 4, SL2_SNAP_TRAJ = 8,
       SL2_SNAP_PARTIAL = 16, SL2_SNAP_PATCHES = 32, SL2_SNAP_ALL = 63 };
/* Host only, no device: upper bound in bytes (a multiple of 16) of ONE blob of an engine of this shape (sl2_create's max_features;
 * params.max_features_to_init_at_once; params.number_of_particles rounded up to 64) restricted to `sections`; with SL2_SNAP_ALL
 * it equals sl2_snapshot_capacity of such an engine.  0 for a bad argument (a negative one, section bits outside SL2_SNAP_ALL). */
size_t sl2_snapshot_bound(int max_features, int partial_slots, int particle_capacity, int sections);
int sl2_snapshot_batch(sl2_engine* e, int seq0, int nseq, int sections, const int32_t* cursors,
                       void* out, size_t out_bytes, uint64_t* offsets, int on_device);

/* ---- annotated frames: the reference's raw-image display for a range of sequences (additions within SL2_API_VERSION 5) ----
 *
 * GraphicTool::DrawRawAR (graphic/graphictool.cpp:285-364) draws, over the camera frame, the 3-sigma search ellipse of every
 * selected feature, each feature's 11 x 11 template where it was matched or is now predicted, the ellipses of a partially
 * initialised feature's particles and the initialisation boxes.  Its numerical half is a DRAW LIST per sequence and a RASTERISER;
 * both run on the device for a whole batch (k_overlay_list, k_overlay_draw: sl2_overlay.hip).
 *
 * THE ITEM, 64 bytes:
 *   kind    SL2_ITEM_RING, SL2_ITEM_PATCH or SL2_ITEM_RECT (and SL2_ITEM_SEGMENT: "the rectified view", below)
 *   label   the feature's label; -1 for a box
 *   a[4]    RING, PATCH: the centre (a[0], a[1]), the rest 0.  RECT: the inclusive corners x0, y0, x1, y1.
 *   patch   PATCH: index into the call's `patches` array, entry k at patches + k * patch_stride, 121 bytes of it used
 *           (row-major 11 x 11); else -1
 *   rgb     the colour;  pad  0
 *   q[4]    RING: A, B, C, rhs; else 0
 *
 * THE PIXEL RULES.  The output is RGB24, [image][height][width][3].  Its base is the grey frame replicated (R = G = B).  A pixel
 * takes the colour of the LAST item in list order that covers it (painter's order: the reference's draw order).  Everything is
 * clipped to the image.  An item of unknown kind, or with a patch index outside the array, draws nothing.
 *   RING   inside(du, dv) := ((A*du)*du + (B*du)*dv) + (C*dv)*dv < rhs, evaluated in FP64 in exactly this order, without
 *          contraction into fused multiply-adds, du and dv being integers converted to double.  The item covers
 *          (a[0] + du, a[1] + dv) iff inside(du, dv) holds and not all of inside(du-1, dv), inside(du+1, dv), inside(du, dv-1),
 *          inside(du, dv+1) hold: the one-pixel rim of the ellipse's interior.  The neighbours are evaluated arithmetically, off
 *          the image too (an ellipse that leaves the image is not closed along the border).  A ring is drawn only if all four q
 *          are finite and A > 0, C > 0, (4.0*A)*C - B*B > 0, rhs > 0.  (The implementation walks a bounding box; the box is
 *          conservative - the set above is the contract, not the box.)
 *   PATCH  with du = x - a[0], dv = y - a[1]: |du| <= 5 and |dv| <= 5: grey patch[(dv+5)*11 + du+5] as R = G = B;
 *          max(|du|, |dv|) == 6: rgb (a frame around the template).
 *   RECT   the one-pixel outline of [x0, x1] x [y0, y1].  An inverted rectangle (x0 > x1 or y0 > y1) draws nothing.
 *   Coordinates are meant to lie within +-32767 (what the list below produces).  Beyond +-2^20 a rectangle's corner counts as
 *   +-2^20 (it clips the same) and a ring or patch centred there draws nothing.  Images are at most 32768 pixels a side.
 *
 * THE DRAW LIST OF A SEQUENCE, in feature_list_ order (DrawRawAR's loop), from the sequence's CURRENT state.  `layers` holds the
 * example's three checkboxes as bits.  Colour (SetFeatureColour, graphictool.cpp:1344): label == marked: green (0,255,0); else
 * selected and matched: red (255,0,0); selected, not matched: blue (0,0,255); otherwise yellow (255,255,0).
 *   fully initialised live feature: zeroedyi and the projection hi are taken from the current xv_, y_ and the sequence's own
 *     camera (sl2_set_cameras).  Only if zeroedyi[2] > 0 (the reference's test against features behind the camera):
 *       SL2_OVERLAY_SEARCH_REGIONS and selected_flag_: a RING at (int(h_[0] + 0.5), int(h_[1] + 0.5)) - the stored h_ and S_ of
 *         the last measurement, C truncation as in elliptical_search - with A = S11, B = -(S01 + S10), C = S00,
 *         rhs = 9.0 * (S00*S11 - S01*S10): the 3-sigma ellipse nu^T S^-1 nu < 9 multiplied through by det S, no division.
 *       SL2_OVERLAY_DESCRIPTORS: a PATCH at (int(x + 0.5), int(y + 0.5)), (x, y) = z_ if selected and matched, else hi.
 *   partially initialised feature, SL2_OVERLAY_SEARCH_REGIONS: the reference's counter (graphictool.cpp:716-733) picks the
 *     particles: step = max(n / 10, 1), particle k (from 0) is drawn iff (k + 1) % step == 0 - at most 19 of them.  Each is a
 *     yellow RING (green if the label is the marked one) at int(m_h_ + 0.5) with A = m_SInv00, B = 2.0 * m_SInv01, C = m_SInv11, rhs = 9.0.  These are the
 *     records of the last MatchPartiallyInitialisedFeatures: the reference recomputes h and S of every drawn particle from the
 *     updated state; this list draws what was SEARCHED.  A particle never predicted carries zeros: its ring is listed and draws
 *     nothing.
 *   SL2_OVERLAY_INITIALISATION, after the features: location_selected_flag_: a green RECT (uu-6, vv-6, uu+6, vv+6);
 *     init_feature_search_region_defined_flag_: a green RECT of the region's four numbers (ustart, vstart, ufinish, vfinish).
 *   A centre that is not finite, or that rounds outside +-32767, omits its item.  Deleted and retired slots yield nothing.
 *   An item's `patch` is (seq - seq0) * max_features + k, k = the feature's index in sl2_get_features order: a client that fills
 *   patches[nseq * max_features][patch_stride] from sl2_get_feature_patch can hand list and array to sl2_draw_items_batch.
 *   No list is longer than sl2_overlay_item_bound(max_features, partial_slots) = 2 max_features + 19 partial_slots + 2.
 *
 * sl2_overlay_items   the lists themselves, for clients that draw vectors: list i (sequence seq0 + i) at items + i * item_stride
 *   (item_stride in items, at least the bound), its length in counts[i].  marked: [nseq] labels, NULL = none marked.
 *   on_device == 0: items, counts, marked are host memory; engine-owned staging (grown on first use), one wait.
 *   on_device != 0: all three are device pointers (items 8-byte aligned); one launch on the engine's stream, no wait.
 * sl2_draw_overlays   list and draw in one call with no host round trip; the templates are the engine's own.  frames: one grey
 *   image per sequence of the range at frames + i * seq_stride (host or device: frames_on_device), engine geometry.  out: RGB24
 *   image i at out + i * out_stride (bytes).  out_on_device == 0: out and marked are host memory; the images are drawn into
 *   engine-owned staging that grows on first use, then one wait and one copy of exactly 3 width height bytes per image.
 *   out_on_device != 0: out and marked are device pointers; two launches on the engine's stream.  With device frames the call
 *   never waits for the device.  With HOST frames (frames_on_device == 0) it waits once, before the launches, until the frames
 *   have been copied into staging - the stream's earlier work included - so that the caller's buffer, which may be pageable, is
 *   free when the call returns; what is drawn afterwards is still not waited for.  Hand over device frames to avoid the wait.
 * Both drop no captured step, change nothing in the engine, do not consult the active mask (a paused sequence is drawn like any
 * other) and work with sequence groups (sl2_set_groups > 1).
 * sl2_draw_items_batch   the stateless rasteriser: `nimages` frames and lists, any mix of host and device residency (patches
 *   lives where the lists live).  Everything on the device: one launch on `stream`, no wait.  Otherwise host inputs are copied
 *   to temporaries and the call waits for `stream` before it returns; that form allocates and frees its temporaries on every
 *   call (tests, tools, a frame now and then).  Only the all-device form is meant for per-frame use.
 * sl2_draw_items_host    the plain C++ form of one image, built from the same source as the kernel: byte for byte its output.
 * Refused (SL2_ERR_INVALID, nothing queued, sl2_last_error() names the sequence or image, or the range where all share the fault): null pointers, ranges outside the
 * batch, nseq or nimages < 1, width or height outside 1 .. 32768, layers with unknown bits, out_stride < 3 width height,
 * seq_stride < width height, item_stride below the bound (sl2_overlay_items) or negative, patch_stride < 121 with npatches > 0;
 * in the HOST-resident lists of sl2_draw_items_batch counts[i] < 0 or > item_stride, an item of unknown kind, a PATCH whose index
 * is outside the array.  A device-resident list cannot be looked at: the kernel clamps its count to 0 .. item_stride and skips
 * such items (they draw nothing, as the pixel rules say, and so they do in sl2_draw_items_host, which is the kernel's arithmetic
 * on the host); every loop is bounded by the clamped count and the image. */
enum { SL2_ITEM_RING = 1, SL2_ITEM_PATCH = 2, SL2_ITEM_RECT = 3, SL2_ITEM_SEGMENT = 5 /* below; 4 is not a kind */ };
enum { SL2_OVERLAY_SEARCH_REGIONS = 1, SL2_OVERLAY_DESCRIPTORS = 2, SL2_OVERLAY_INITIALISATION = 4, SL2_OVERLAY_ALL = 7 };
typedef struct sl2_overlay_item {
  int32_t kind;
  int32_t label;
  int32_t a[4];
  int32_t patch;
  uint8_t rgb[3];
  uint8_t pad;
  double q[4];
} sl2_overlay_item;                            /* 64 bytes */
/* Host only, no device: the longest list of a sequence of an engine of this shape; 0 for a negative argument. */
size_t sl2_overlay_item_bound(int max_features, int partial_slots);
int sl2_overlay_items(sl2_engine* e, int seq0, int nseq, int layers, const int32_t* marked /* [nseq] labels, NULL = none */,
                      sl2_overlay_item* items, int item_stride, int32_t* counts, int on_device);
int sl2_draw_items_batch(int device, void* stream, const uint8_t* frames, int frames_on_device, int nimages, int width, int height,
                         size_t seq_stride, const sl2_overlay_item* items, int item_stride, const int32_t* counts,
                         int items_on_device, const uint8_t* patches, size_t patch_stride, int npatches, uint8_t* out,
                         size_t out_stride, int out_on_device);
int sl2_draw_overlays(sl2_engine* e, int seq0, int nseq, const uint8_t* frames, size_t seq_stride, int frames_on_device,
                      int layers, const int32_t* marked, uint8_t* out, size_t out_stride, int out_on_device);
int sl2_draw_items_host(const uint8_t* frame, int width, int height, const sl2_overlay_item* items, int count,
                        const uint8_t* patches, size_t patch_stride, int npatches, uint8_t* out);

/* ---- the rectified view (additions within SL2_API_VERSION 5): a line in the rasteriser, the undistorted frame, the 3-D scene ----
 *
 * GraphicTool::DrawRectifiedAR (graphic/graphictool.cpp:222-283) shows the MAP: the camera frame with the lens distortion
 * removed and, over it, the 3-D features, their uncertainty ellipsoids, the rays of partially initialised features and the
 * trajectory.  Its numerical half is the line primitive that scene needs, the frame (k_rectify), the scene as a DRAW LIST per
 * sequence for the rasteriser above (k_scene_list), and the three chained (sl2_draw_rectified); all run on the device for a
 * whole batch (sl2_rectify.hip).
 *
 * SL2_ITEM_SEGMENT = 5, a fourth kind of the item above, in every drawing call above (kind 4 stays unassigned and draws
 * nothing):  a[4] = x0, y0, x1, y1, the two ends;  patch = -1;  q = 0.  THE PIXEL RULE, in integers (64-bit where products
 * need it), no floating point:
 *   each of the four coordinates beyond +-2^20 counts as +-2^20 (as for RECT);
 *   dx = x1 - x0, dy = y1 - y0; the segment is x-major iff |dx| >= |dy|, else y-major;
 *   the two ends are exchanged if that is needed for the major coordinate not to decrease from the first to the second;
 *   x-major, with D = x1 - x0 >= 0 and dy = y1 - y0 after the exchange: the item covers (x, y) iff x0 <= x <= x1 and
 *     y == y0 + floor((2 (x - x0) dy + D) / (2 D)) - the division FLOORED (towards minus infinity), not truncated; with
 *     D == 0 (then dy == 0 too) it covers the one pixel (x0, y0);
 *   y-major: the same with x and y exchanged.
 *   One pixel per step of the major coordinate, the nearest one; where the line passes exactly midway between two pixels
 *   (2 (x - x0) dy + D an exact multiple of 2 D) the one with the larger minor coordinate.  After the exchange a segment and
 *   its reverse are the same item: they cover the same pixels, the ties included.  The set is clipped to the image; the
 *   implementation's box is the ends' box.  The painter's rule is unchanged: the last item wins.
 *
 * sl2_rectify_frames   the frame with the lens distortion removed, for sequences seq0 .. seq0 + nseq - 1 in ONE launch
 *   (k_rectify, sl2_rectify.hip).  frames: one grey image per sequence at frames + i * seq_stride, engine geometry, host or
 *   device memory; out: grey images of the same size at out + i * out_stride.  Sequence seq0 + i is warped with ITS OWN u0, v0
 *   and kd1 as the setters queued so far leave them (sl2_set_cameras), read on the device from the sequence's record: the call
 *   is ordered behind them on the engine's stream.  THE PIXEL RULE, for output pixel (x, y), in FP64, in exactly this order,
 *   without contraction into fused multiply-adds:
 *     cx = x - u0;  cy = y - v0;  r2 = cx*cx + cy*cy;  f = 1.0 + (2.0*kd1)*r2;
 *     !(f > 0): BORDER.  s = sqrt(f);  xs = cx / s + u0;  ys = cy / s + v0      (Camera::Project's distortion, camera.cpp:108-113:
 *       where the ideal pinhole point (x, y) lands in the camera's own image);
 *     xs or ys not finite, or beyond +-2^20: BORDER;
 *     X = floor(xs*32.0 + 0.5), Y = floor(ys*32.0 + 0.5) as integers: the source position in 1/32 pixel;
 *     ix = X >> 5 (floored), fx = X & 31 (0 .. 31), iy and fy likewise; p00 = frame(ix, iy), p10 = frame(ix + 1, iy),
 *     p01 = frame(ix, iy + 1), p11 = frame(ix + 1, iy + 1), a tap off the image reading BORDER;
 *     out = ((32-fx)*(32-fy)*p00 + fx*(32-fy)*p10 + (32-fx)*fy*p01 + fx*fy*p11 + 512) >> 10.
 *   BORDER = 0.  With kd1 == 0 the output is the input.  The output has the INPUT's geometry and principal point and is exact
 *   per pixel; the reference draws a 10 x 10 mesh of textured quads whose outline is the undistorted image border, i.e. it
 *   scales the view so that the whole frame shows.  This call crops instead: what a pinhole camera of the same fku, fkv, u0,
 *   v0 sees within width x height, so a 3-D point X in the camera frame lies at (u0 - fku X0/X2, v0 - fkv X1/X2) of the output.
 *   Residency and waiting are sl2_draw_overlays': host frames are copied into engine-owned staging; in front of a device output
 *   the call waits once, until they have been copied.  A host output is written into staging, then one wait and one copy of
 *   exactly width height bytes per image.  With device frames and a device output: one launch on the engine's stream, no wait.
 *   out must not overlap frames.  The call drops no captured step, changes nothing in the engine, does not consult the active
 *   mask and works with sequence groups.
 * sl2_rectify_frame_host   the plain C++ form of one image from the same source as the kernel (no device needed): byte for
 *   byte its output.  width and height within 1 .. 32768; u0, v0, kd1 finite.
 *
 * THE SCENE'S DRAW LIST OF A SEQUENCE, from its CURRENT state, in DrawRectifiedAR's order.  `layers` holds the example's three
 * checkboxes as bits: SL2_SCENE_TRAJECTORY = 1, SL2_SCENE_FEATURES = 2, SL2_SCENE_UNCERTAINTIES = 4.  The camera of the
 * rectified image is the sequence's own (sl2_set_cameras) with kd1 = 0: a point X of the camera frame (zeroedyi: RRW (y - r)
 * of the current xv_) with X[2] >= 0.01 (kNear_) projects to (u0 - fku X[0]/X[2], v0 - fkv X[1]/X[2]), evaluated as written.
 * Colour and `marked` are SetFeatureColour's, as for the annotated frames above; rounding is int(v + 0.5), C truncation, and a
 * coordinate that is not finite or rounds outside +-32767 omits its item.
 *   A 3-D SEGMENT a .. b of the camera frame becomes an SL2_ITEM_SEGMENT in this order of operations:
 *     (1) both ends with X[2] < 0.01: omitted.  One end behind: with t = (0.01 - a[2]) / (b[2] - a[2]) the point
 *         (a[0] + t (b[0] - a[0]), a[1] + t (b[1] - a[1]), 0.01) replaces it;
 *     (2) both ends are projected (p, r); not finite: omitted;
 *     (3) the 2-D segment is clipped to the guard square [-32767, 32767]^2 by Liang-Barsky - edges in the order left, right,
 *         top, bottom, each a constraint pk t <= qk with pk = -dx, dx, -dy, dy and qk = p[0] + 32767, 32767 - p[0],
 *         p[1] + 32767, 32767 - p[1]; t0 = 0, t1 = 1 tightened by t = qk / pk; entirely outside: omitted; the ends become
 *         p + t0 (dx, dy) and p + t1 (dx, dy);
 *     (4) the four coordinates are rounded.
 *   SL2_SCENE_TRAJECTORY, first: for consecutive entries of trajectory_store_ as sl2_get_trajectory returns them (the up to
 *     1000 most recent, oldest first), the segment between the two, both taken into the camera frame; yellow, label -1.
 *   Then the features in feature_list_ order:
 *   fully initialised live feature, m = zeroedyi:
 *     SL2_SCENE_FEATURES and m[2] >= 0.01: a filled 3 x 3 marker at the rounded projection (x, y), as RECT (x-1, y-1, x+1, y+1)
 *       then RECT (x, y, x, y).
 *     SL2_SCENE_UNCERTAINTIES: Sigma = Pzeroedyigraphics (feature_model.cpp:128-145) from the current P, with Jx =
 *       dzeroedyi_by_dxp (3 x 7; dxp_by_dxv is the identity on the first seven columns), Jy = dzeroedyi_by_dyi = RRW, Pxx the
 *       leading 7 x 7 of P, Pxy its first 7 rows in the feature's columns, Pyy the feature's block.  Summation order (so that
 *       the list is reproducible to the bit): every inner sum starts at 0.0 and runs over its index upwards;
 *       A = Jx Pxx, Bm = Jx Pxy, Cm = Jy Pyy;  T1[i][j] = sum_c A[i][c] Jx[j][c], T3[i][j] = sum_c Bm[i][c] Jy[j][c],
 *       T4[i][j] = sum_c Cm[i][c] Jy[j][c];  Sigma[i][j] = ((T1[i][j] + T3[j][i]) + T3[i][j]) + T4[i][j].
 *       The outline of the 3-sigma ellipsoid under the pinhole is a conic: D[i][j] = m[i]*m[j] - 9.0*Sigma[i][j] (entries 00,
 *       01, 02, 11, 12, 22 from Sigma's 00, 01, 02, 11, 12, 22), d = D22.  Only if d > 0 and m[2] > 0 (the ellipsoid lies wholly
 *       in front of the camera plane; d > 0 alone holds for one wholly behind it too): cn = (D02/d, D12/d); En00 = cn0*cn0 - D00/d, En01 = cn0*cn1 - D01/d, En11 = cn1*cn1 - D11/d;
 *       E00 = (fku*En00)*fku, E01 = (fku*En01)*fkv, E11 = (fkv*En11)*fkv; a RING at the rounded (u0 - fku*cn0, v0 - fkv*cn1)
 *       with A = E11, B = -2.0*E01, C = E00, rhs = E00*E11 - E01*E01.  A form that is not positive definite is listed and
 *       draws nothing (the RING's own rule).
 *   partially initialised feature, SL2_SCENE_FEATURES: the ray y0 .. y0 + 10.0 hhat (kSemiInfiniteLineLength_) of the partial
 *     model's zeroed state (y0 = RRW (r_i - r), hhat = RRW hhat_i), as a 3-D segment above, with the feature's label and
 *     colour.  (The reference draws no uncertainty on lines.)
 *   Left out: DrawAxes - its extents are accumulators of the GL drawing state, not of the map.
 *   No list is longer than sl2_scene_item_bound(max_features, partial_slots) = 3 max_features + partial_slots + 999.
 *
 * sl2_scene_items    the lists themselves; arguments, residency and waiting as sl2_overlay_items (items of a device list
 *   8-byte aligned, item_stride at least sl2_scene_item_bound).  sl2_draw_items_batch accepts the lists as they are (no patches).
 * sl2_draw_rectified rectify, list and draw with no host round trip: three stream-ordered launches (k_rectify into
 *   engine-owned staging, k_scene_list, k_overlay_draw over the rectified grey).  Arguments, residency and waiting as
 *   sl2_draw_overlays; out is RGB24.  Both drop no captured step, change nothing in the engine, do not consult the active
 *   mask and work with sequence groups.
 * Refused (SL2_ERR_INVALID, nothing queued, sl2_last_error() names the sequences): null pointers, a range outside the batch,
 * nseq < 1, layers with bits outside SL2_SCENE_ALL, seq_stride below width height, out_stride below width height
 * (sl2_rectify_frames) or 3 width height (sl2_draw_rectified), item_stride below the bound, a misaligned device `items`; in the
 * host form a null pointer, a size outside 1 .. 32768 or a camera number that is not finite. */
enum { SL2_SCENE_TRAJECTORY = 1, SL2_SCENE_FEATURES = 2, SL2_SCENE_UNCERTAINTIES = 4, SL2_SCENE_ALL = 7 };
int sl2_rectify_frames(sl2_engine* e, int seq0, int nseq, const uint8_t* frames, size_t seq_stride, int frames_on_device,
                       uint8_t* out, size_t out_stride, int out_on_device);
int sl2_rectify_frame_host(const uint8_t* frame, int width, int height, double u0, double v0, double kd1, uint8_t* out);
/* Host only, no device: the longest scene list of a sequence of an engine of this shape; 0 for a negative argument. */
size_t sl2_scene_item_bound(int max_features, int partial_slots);
int sl2_scene_items(sl2_engine* e, int seq0, int nseq, int layers, const int32_t* marked /* [nseq] labels, NULL = none */,
                    sl2_overlay_item* items, int item_stride, int32_t* counts, int on_device);
int sl2_draw_rectified(sl2_engine* e, int seq0, int nseq, const uint8_t* frames, size_t seq_stride, int frames_on_device,
                       int layers, const int32_t* marked, uint8_t* out, size_t out_stride, int out_on_device);

/* ---- the world view and picking (additions within SL2_API_VERSION 5): the 3-D scene from a free camera ----
 *
 * GraphicTool::Draw3dScene (graphic/graphictool.cpp:113-175) shows the map, the trajectory and the camera FROM OUTSIDE, through a
 * movable virtual camera; GraphicTool::Picker (1475-1571) answers which feature lies under a click.  Their numerical half is a
 * DRAW LIST per sequence for the rasteriser above (k_world_list) and a query over any draw list (k_pick_items), both for a
 * whole batch (sl2_world_view.hip).  No new item kind: RECT, RING and SEGMENT only.
 *
 * THE VIEW, sl2_view, 88 bytes: a pinhole camera posed in the world with the reference's conventions, r its position, q = qWR
 * (w, x, y, z) used AS GIVEN (not normalised: Eigen's inverse() and toRotationMatrix(), as for xv_).  A world point Y has
 * view-frame coordinates X = zeroedyi((r, q), Y) = RRW (Y - r), the expressions of the sequence's own camera frame, and a
 * point with X[2] >= 0.01 lies at (u0 - fku X[0]/X[2], v0 - fkv X[1]/X[2]), evaluated as written.
 * sl2_view_look_at   host only: the view at `eye` whose frame has z towards `target`, x = up x z normalised (image LEFT) and
 *   y = z x x (image UP), as a unit quaternion with q[0] >= 0.  A point displaced along `up` lands at a smaller v, one to the
 *   viewer's right at a larger u, the target at (u0, v0).  Refused: a null pointer, a number that is not finite, eye == target,
 *   `up` zero or parallel to the viewing direction (|up x z| <= 1e-12 |up|).  The reference example's view is
 *   eye (0, 0.18, -1.4), target (0, 0.13, 0), up (0, 1, 0) (ModelViewLookAt, pangolin_util.cpp) with the camera's intrinsics.
 *
 * THE WORLD'S DRAW LIST OF A SEQUENCE, from its CURRENT state, in Draw3dScene's order.  `layers`: SL2_WORLD_TRAJECTORY = 1,
 * SL2_WORLD_FEATURES = 2, SL2_WORLD_UNCERTAINTIES = 4 (the example's three check boxes), SL2_WORLD_CAMERA = 8, SL2_WORLD_AXES = 16
 * (the reference always draws the camera, and the axes with the features box).  Colour, `marked`, rounding (int(v + 0.5), C
 * truncation; not finite or outside +-32767 omits the item) and the rule of a 3-D SEGMENT (steps (1) to (4): near plane 0.01,
 * projection, Liang-Barsky to the guard square, rounding) are those of the rectified view above, word for word, with the VIEW
 * in the place of the sequence's camera: "into the view frame" below is X = RRW (Y - r) of the view.
 *   SL2_WORLD_CAMERA, first (DrawCamera, drawn as wire): 16 segments, colour (150, 150, 150), label -1.  The glyph's frame is
 *     the world turned by qWO = qWR * (0, 0, 1, 0) = (-qy, -qz, qw, qx) of the current xv_'s (qw, qx, qy, qz), at r of xv_: a
 *     glyph point g is the world point W[i] = r[i] + ((0.0 + R[i][0] g[0]) + R[i][1] g[1]) + R[i][2] g[2], R =
 *     toRotationMatrix(qWO) without normalisation, and W is then taken into the view frame.  Edges 0 .. 11 are the body box
 *     x in {-0.032, 0.026}, y in {-0.034, 0.020}, z in {-0.012, 0.012} (lensposx, lensposy, width, height, depth), a corner
 *     written (bx, by, bz) with bit 0 = the lower and 1 = the upper value: edge e = 0 .. 3 runs along x from (0, e & 1, e >> 1)
 *     to (1, e & 1, e >> 1); edge 4 + e along y from (e & 1, 0, e >> 1) to (e & 1, 1, e >> 1); edge 8 + e along z from
 *     (e & 1, e >> 1, 0) to (e & 1, e >> 1, 1).  Edges 12 .. 15 are the lens's front face at z = -0.017, corners c0 .. c3 =
 *     (-0.012, -0.012), (0.012, -0.012), (0.012, 0.012), (-0.012, 0.012): edge 12 + k from ck to c((k + 1) % 4).
 *   SL2_WORLD_TRAJECTORY: consecutive entries of trajectory_store_ as sl2_get_trajectory returns them, both into the view
 *     frame, the 3-D segment between them; yellow, label -1.
 *   Then the features in feature_list_ order (one loop, as in Draw3dScene):
 *   fully initialised live feature, m = y into the view frame:
 *     SL2_WORLD_FEATURES and m[2] >= 0.01: the filled 3 x 3 marker at the rounded projection, RECT (x-1, y-1, x+1, y+1) then
 *       RECT (x, y, x, y).
 *     SL2_WORLD_UNCERTAINTIES: the world-frame ellipsoid (func_yigraphics_and_Pyiyigraphics: y_ and Pyy_ alone, no camera
 *       uncertainty) in the view frame: Sigma = (Jy Pyy) Jy^T, Jy = RRW of the view, Pyy the feature's block of the current P;
 *       every inner sum starts at 0.0 and runs over its index upwards: Cm[i][c] = sum_k Jy[i][k] Pyy[k][c],
 *       Sigma[i][j] = sum_c Cm[i][c] Jy[j][c].  Then the conic of the rectified view above from (m, Sigma) and the view's fku,
 *       fkv, u0, v0, under the same conditions (d > 0 and m[2] > 0): a RING.
 *   partially initialised feature, SL2_WORLD_FEATURES: the ray r_i .. r_i + 10.0 hhat_i of its state IN THE WORLD
 *     (b[k] = r_i[k] + 10.0 * hhat_i[k]), both ends into the view frame, a 3-D segment with the feature's label and colour.
 *   SL2_WORLD_AXES, last (DrawAxes without letters, tick numbers and lighting): the EXTENTS xmin, xmax, ymin, ymax, zmin, zmax
 *     start at 0.0 and take in (v < min: min = v; v > max: max = v, per coordinate) r of xv_ and, with SL2_WORLD_FEATURES set,
 *     y of every fully initialised live feature (UpdateDrawingDimension, graphictool.cpp:126, 138, 155).  Three white segments
 *     (255, 255, 255), label -1, both ends into the view frame: (xmin,0,0)..(xmax,0,0), (0,ymin,0)..(0,ymax,0),
 *     (0,0,zmin)..(0,0,zmax).
 *   No list is longer than sl2_world_item_bound(max_features, partial_slots) = 3 max_features + partial_slots + 999 + 19.
 *
 * sl2_world_items   the lists; items, item_stride, counts, marked as sl2_scene_items.  views: nviews == 1 (one view for all
 *   sequences) or nviews == nseq (view i for sequence seq0 + i).  extents: [nseq][6] doubles or NULL - the EXTENTS above,
 *   computed whether or not SL2_WORLD_AXES is among the layers: a client fits its next view with them.  on_device == 0: views,
 *   marked, items, counts, extents are host memory; engine-owned staging, one wait.  on_device != 0: all are device pointers
 *   (items and views 8-byte aligned); one launch on the engine's stream, no wait.
 * sl2_draw_world    fill, list and draw with no host round trip: engine-owned staging of nseq grey images of width x height
 *   (ANY size within 1 .. 32768, not the engine's) is filled with the grey level `background` (0 .. 255), then k_world_list,
 *   then k_overlay_draw; all stream-ordered.  out: RGB24 image i at out + i * out_stride.  out_on_device == 0: views, marked
 *   and out are host memory, one wait and one copy of exactly 3 width height bytes per image.  out_on_device != 0: all three
 *   are device pointers and the call never waits.
 * Both drop no captured step, change nothing in the engine, do not consult the active mask and work with sequence groups.
 * Refused (SL2_ERR_INVALID, nothing queued, sl2_last_error() names the call and the sequences): null pointers, a range outside
 * the batch, nseq < 1, nviews other than 1 or nseq, layers with bits outside SL2_WORLD_ALL, item_stride below the bound, device
 * items or views not 8-byte aligned, width or height outside 1 .. 32768, background outside 0 .. 255, out_stride below
 * 3 width height, a HOST-resident view with a number that is not finite (the sequence is named).  A device-resident view cannot
 * be looked at: one with a number that is not finite lists nothing it touches and cannot fault - every rule above omits an
 * item whose coordinates are not finite, and every store is bounded by item_stride.
 *
 * PICKING (GraphicTool::Picker: gluPickMatrix(x, y, 7, 7) over the names of the drawn features).  The window is the 7 x 7 pixels
 * centred on the click (x, y), clipped to the image.  The answer is the LAST item in list order with label >= 0 that covers,
 * by THE PIXEL RULES above, at least one pixel of the window: picked = (its label, its index in the list); (-1, -1) if there
 * is none.  Items with label -1 neither count nor hide anything (coverage, not visibility: a labelled item under an unlabelled
 * one is still picked).  A PATCH covers its 13 x 13 square whatever its template holds.  An item that draws nothing (unknown
 * kind, a ring that fails its own rule, a patch index outside 0 .. npatches - 1, an inverted rectangle) is never picked.  A
 * click outside the image answers (-1, -1); it is not refused.  The adapters return label + 1, the reference's GL name.
 * sl2_pick_items_batch   list i at items + i * item_stride with counts[i] items, click i = clicks[2 i], clicks[2 i + 1],
 *   answer i in picked[2 i], picked[2 i + 1].  on_device != 0: items (8-byte aligned), counts, clicks and picked are device
 *   pointers; one launch on `stream` (k_pick_items), no wait; a count is clamped to 0 .. item_stride.  on_device == 0: all four
 *   are host memory; the lists are checked as sl2_draw_items_batch checks them (a count outside 0 .. item_stride, an unknown
 *   kind or a patch index outside the array is refused, the image named), copied to temporaries, and the call waits.
 * sl2_pick_items_host    the plain C++ form of one image from the same source as the kernel (no device needed); nothing is
 *   refused of the items.
 * Refused: null pointers, nimages < 1, width or height outside 1 .. 32768, item_stride, count or npatches negative, misaligned
 * device items. */
enum { SL2_WORLD_TRAJECTORY = 1, SL2_WORLD_FEATURES = 2, SL2_WORLD_UNCERTAINTIES = 4, SL2_WORLD_CAMERA = 8, SL2_WORLD_AXES = 16,
       SL2_WORLD_ALL = 31 };
typedef struct sl2_view {
  double r[3];              /* position in the world */
  double q[4];              /* qWR (w, x, y, z), used as given */
  double fku, fkv, u0, v0;
} sl2_view;                                    /* 88 bytes */
int sl2_view_look_at(const double eye[3], const double target[3], const double up[3], double fku, double fkv, double u0, double v0,
                     sl2_view* out);
/* Host only, no device: the longest world list of a sequence of an engine of this shape; 0 for a negative argument. */
size_t sl2_world_item_bound(int max_features, int partial_slots);
int sl2_world_items(sl2_engine* e, int seq0, int nseq, const sl2_view* views, int nviews, int layers, const int32_t* marked,
                    sl2_overlay_item* items, int item_stride, int32_t* counts, double* extents /* [nseq][6] or NULL */, int on_device);
int sl2_draw_world(sl2_engine* e, int seq0, int nseq, const sl2_view* views, int nviews, int width, int height, int background,
                   int layers, const int32_t* marked, uint8_t* out, size_t out_stride, int out_on_device);
int sl2_pick_items_batch(int device, void* stream, int nimages, int width, int height, const sl2_overlay_item* items, int item_stride,
                         const int32_t* counts, int npatches, const int32_t* clicks /* [nimages][2] x, y */,
                         int32_t* picked /* [nimages][2] label, item index */, int on_device);
int sl2_pick_items_host(int width, int height, const sl2_overlay_item* items, int count, int npatches, int x, int y, int32_t picked[2]);

/* selected_feature_list_ (labels, selection order) and per-step counters:
 * counters[0] = number_of_visible_features_, [1] = #selected,
 * [2] = successful_measurement_vector_size_. */
int sl2_get_selection(sl2_engine* e, int seq, int32_t* labels, int capacity, int32_t counters[3]);
/* trajectory_store_ (monoslam.cpp:172-177; keeps the reference's stale-scratch
 * behaviour): up to `capacity` most recent entries of 3 doubles. */
int sl2_get_trajectory(sl2_engine* e, int seq, double* out, int capacity, int* count);
/* xv_(0..2) after each of the last `count` steps (the actual camera trajectory; the
 * reference's trajectory_store_ holds a stale scratch value instead):
 * out [nseq][count][3], count = min(capacity, steps done, 1000). */
int sl2_get_position_log(sl2_engine* e, int seq0, int nseq, double* out, int capacity, int* count);
/* MonoSLAM::mark_feature_by_lab(label) + delete_feature() (monoslam.cpp:743-812) for one feature per sequence:
 * labels [nseq], -1 = leave that sequence alone.  deleted [nseq] (may be NULL) receives the reference's bool: 1 if a live,
 * fully initialised feature with that label existed and was removed (partially initialised ones are removed by the engine's
 * own sell-by / conversion logic only).  The label is never reused (its slot may be).  Synchronises. */
int sl2_delete_features(sl2_engine* e, int seq0, int nseq, const int32_t* labels, int32_t* deleted);
/* Per-sequence status bits.  SL2_STATUS_NONFINITE (sticky): NaN / Inf seen in the state (e.g. the omega == 0 hazard, Q10).
 * SL2_STATUS_LABELS_EXHAUSTED: the LAST feature initialisation that was called for (speed gate and visible-feature count of
 * GoOneStep, or one of the two initialise-feature entry points) could not take place because every one of the sequence's
 * max_features slots holds a LIVE feature (the reference's feature_list_ is unbounded).  Deleted features do not count:
 * their slots are squeezed out, in feature_list_ order, when a sequence runs out of slots, and labels (Feature::label_ =
 * next_free_label_++) are kept apart from slots and never reused - a sequence may hand out any number of labels over its
 * lifetime.  The bit is cleared again by the next initialisation attempt that finds room (after a feature has been deleted),
 * so a temporarily full map is not a permanent condition.  While it is set the sequence keeps tracking its map but
 * initialises no further features.  Callers that run with enable_mapping must poll this (the MonoSLAM adapters do, and
 * raise when the bit RISES). */
#define SL2_STATUS_NONFINITE 1
#define SL2_STATUS_LABELS_EXHAUSTED 2
/* SL2_STATUS_REFERENCE_OUT_OF_BOUNDS (sticky): the position the reference records for a feature after several conversions in
 * front of it and deletions (feature.cpp:254, Q28; see sl2_go_one_step for how a position becomes misplaced) has gone
 * NEGATIVE; the reference then writes its dh_by_dy block outside dh_by_dx_tot (monoslam.cpp:564, undefined behaviour).  The
 * engine holds the block at column 0 and flags the sequence: from here on its filter is not the reference's. */
#define SL2_STATUS_REFERENCE_OUT_OF_BOUNDS 4
/* SL2_STATUS_SMALL_STEP_REFUSED (sticky): the fused small-map update was launched for a sequence it cannot take (a live map
 * wider than its LDS panel, or a dh_by_dy block outside the live state) and skipped that sequence's Kalman update instead of
 * reaching outside its memory.  Never expected: the engine chooses the fused step only for maps it fits, so the bit means an
 * engine bug, and the sequence's filter is no longer the reference's. */
#define SL2_STATUS_SMALL_STEP_REFUSED 8
int sl2_get_status_flags(sl2_engine* e, int seq0, int nseq, int32_t* flags);

/* The filter-consistency record of the last completed update, for a range of sequences in ONE launch (an addition within
 * SL2_API_VERSION 5).  "Update" = the Kalman update of sl2_go_one_step in every form (ten, six or three launches, captured or
 * not) or of the seams sl2_make_measurements + sl2_kalman_filter_update.  The update leaves w = L^-1 nu (S = L L^T the joint
 * innovation covariance of the matched features, nu the stacked innovation) and the diagonal of L^-1 in its workspaces; one
 * wavefront per sequence forms the record from them on demand (k_step_stats, sl2_stats.hip), FP64 throughout, in a fixed order:
 * the bytes of a sequence's record do not depend on seq0, nseq, the host or device form, sequence groups, graph replay or how
 * often the call is made.  A step pays nothing for it when nobody asks.
 *   nis        = nu^T S^-1 nu = sum w_r^2: chi-square with `dof` degrees of freedom for a consistent filter.  The bounds are
 *                the caller's business (a table, scipy.stats.chi2); the library ships none.
 *   log_det_S  = 2 sum log L_rr (a log per pivot, summed): -(nis + log_det_S + dof log 2 pi) / 2 is the step's log-likelihood.
 *   min_pivot, max_pivot = min / max L_rr, taken as 1 / (L^-1)_rr (the factorisation keeps L's diagonal blocks on chip and
 *                writes their inverses): (max / min)^2 is a lower bound of cond(S).
 *   worst_label, worst_feature_d2 = the matched feature with the largest OWN nu_i^T S_i^-1 nu_i (its 2 x 2 S_i and nu_i as
 *                sl2_feature_info reports them; ties go to the earlier feature of feature_list_) - the first candidate for
 *                sl2_delete_features when nis is out of bounds.
 * stepped = 0 for a sequence the update did not run for - paused (sl2_set_active_sequences) in the last step; not stepped since
 * sl2_create / sl2_load_sequences / sl2_copy_sequences (destination) / sl2_reset_sequences; or refused
 * (SL2_STATUS_SMALL_STEP_REFUSED) - then dof = 0, worst_label = -1 and the doubles except position_var are zero, while the
 * counts, status_flags and sequence_steps are live.  An active sequence without a match has stepped = 1, dof = 0.  The record is
 * STALE between sl2_make_measurements and sl2_kalman_filter_update (dof is the new frame's, w the old one's): ask after the
 * update.  position_var is read at query time.
 * out_on_device == 0: one launch into a pinned buffer of the engine's, one stream synchronisation, a copy into out[nseq].
 * out_on_device != 0: out is device memory (8-byte aligned); the launch only, on the engine's stream, no synchronisation - a
 * kernel of the caller's on that stream, or sl2_set_active_sequences(on_device = 1), can consume it.  Never drops a captured step. */
typedef struct sl2_step_stats {        /* 96 bytes, 8-byte aligned */
  int32_t stepped;          /* 1 = the sequence took part in the last update (active, and stepped since it was loaded / copied in / reset) */
  int32_t status_flags;     /* SL2_STATUS_* */
  int32_t sequence_steps;   /* as sl2_snapshot_header.sequence_steps */
  int32_t n_features;       /* as sl2_snapshot_header.n_features */
  int32_t n_partial;
  int32_t n_visible, n_selected, n_matched;   /* number_of_visible_features_, selected_feature_list_.size(), successful features */
  int32_t dof;              /* rows of the innovation system the update solved: 2 * n_matched, 0 when no update ran */
  int32_t worst_label;      /* label of the matched feature with the largest own nu_i^T S_i^-1 nu_i; -1 if none */
  double nis;               /* nu^T S^-1 nu of the joint system */
  double log_det_S;
  double min_pivot, max_pivot;   /* min / max L_rr */
  double worst_feature_d2;  /* that feature's nu_i^T S_i^-1 nu_i, from f_nu and f_S */
  double position_var;      /* Pxx(0,0) + Pxx(1,1) + Pxx(2,2) after the step */
  int32_t reserved[2];
} sl2_step_stats;
int sl2_get_step_stats(sl2_engine* e, int seq0, int nseq, sl2_step_stats* out, int out_on_device);

/* ------------------------------------------------- save / restore / copy / reset of sequences */

/* The COMPLETE state of one sequence as a self-describing, position-independent blob (additions within SL2_API_VERSION 5): not
 * the public view of sl2_snapshot but everything a later step reads - x and P, templates in their packed form, retired slots,
 * counters, the recorded-position offsets (Q28), the partially initialised features with their particles, the drand48 state,
 * both trajectory stores.  k_seq_pack / k_seq_unpack (sl2_checkpoint.hip) write and read it on the device.  A blob can be loaded
 * into any sequence of any engine that FITS: the destination SEQUENCE's sl2_camera (sl2_set_cameras; the sl2_create camera unless
 * set) equal to the one the blob records, the same sl2_params (bytewise, except max_features_to_init_at_once
 * and number_of_features_to_select, which must be at least what the blob uses: its partial slots, its selected features),
 * max_features >= n_slots, partial slots >= n_partial_slots, particle capacity >= n_particles.  Same-shape engines continue a
 * loaded sequence bit for bit; another shape keeps every integer result and agrees to rounding (the partial features' columns
 * sit elsewhere, so sums run in another order).
 *
 * Layout: every section starts on a 64-byte boundary at the offset the header gives.  n = 13 + 3 n_slots + 6 n_partial_slots.
 *   header        sl2_sequence_blob_header (256 bytes), written LAST by the device
 *   off_x         double[row_pitch]            canonical order: vehicle (13), slots 0 .. n_slots - 1 (3 each, retired slots
 *                                              included: they are zero), partial slots 0 .. n_partial_slots - 1 (6 each); zero padded
 *   off_P         double[n][row_pitch]         the leading n x n square in the same order (the full square, not a triangle: P is
 *                                              symmetric only after sl2_finish_step); row_pitch = n rounded up to 8 doubles
 *   off_slots     SL2_BLOB_SLOT_ARRAYS arrays of [n_slots] records, each array on a 64-byte boundary, in this order (bytes per
 *                 record): template 288, patch_sums 8, xp_org 64, flags 4, label 4, attempted 4, successful 4, pos_err 4,
 *                 h column 4 (canonical column), h 16, Hx 112, Hy 48, R 8, S 32, score 8, z 16, nu 16, selection order 4,
 *                 meas_ok 4, meas_score 8, successes 4, first row in S 4   (sl2_sequence_blob_layout reports each offset)
 *   off_seq       448 bytes: int32 n_slots, next_label, status, pos_err_any, n_selected, n_visible, m_count, traj_count;
 *                 uint64 drand48 state; double prev_r[3], last_r[3], part_d[4]; at 128: int32 part_i[16]; at 192: int32
 *                 ps_i[4][8]; at 320: double ps_d[4][4]
 *   off_particles double[n_partial_slots][n_particles][12]
 *   off_traj      double[1000][3]  trajectory_store_ ring (entry k of the sequence's life at k % 1000)
 *   off_pos_log   double[1000][3]  the position log, oldest first, the newest entry LAST; entries from before the sequence
 *                                  existed are zero
 * Not in the blob: what a step rewrites before it reads it (search windows, A^T, V^T, S, L, the particles' search ellipses, the
 * score cache, the work counters).  A blob is therefore taken between steps, or between the seams from sl2_make_measurements on.
 *
 * The step clock: an engine counts steps, not its sequences.  A loaded or reset sequence takes the DESTINATION engine's step
 * index; its position log is placed so that its newest entry is the destination's newest, and sl2_get_position_log shows of it
 * what is not older than the destination engine (count = min(capacity, destination steps done, 1000)).  The sequence's own age
 * travels in the header and is reported by sl2_snapshot_header.sequence_steps. */
#define SL2_BLOB_MAGIC 0x51324c53u /* "SL2Q" */
#define SL2_BLOB_LAYOUT_VERSION 1
#define SL2_BLOB_SLOT_ARRAYS 22
typedef struct sl2_sequence_blob_header {
  uint32_t magic;                              /* SL2_BLOB_MAGIC */
  uint32_t layout_version;                     /* SL2_BLOB_LAYOUT_VERSION */
  uint64_t bytes;                              /* size of the whole blob, a multiple of 64 */
  int64_t sequence_steps;                      /* steps the sequence has taken */
  int32_t src_max_features, src_partial_slots, src_particle_capacity;   /* shape of the engine that wrote it */
  int32_t width, height;
  int32_t n_slots;                             /* feature slots in use (live, reserved or retired) */
  int32_t n_partial_slots;                     /* highest partial slot in use + 1 */
  int32_t n_particles;                         /* particles stored per partial slot (the largest count in use) */
  int32_t mapping_in_use;                      /* the source engine had feature initialisation in use */
  uint32_t off_x, off_P, off_slots, off_seq, off_particles, off_traj, off_pos_log;
  int32_t row_pitch;                           /* doubles per row of x / P in the blob */
  int32_t state_size;                          /* n */
  sl2_camera camera;                           /* the calibration the SEQUENCE ran under (sl2_set_cameras) */
  sl2_params params;
  int32_t n_selected;                          /* features selected in the sequence's last selection (rows of the innovation system) */
  int32_t reserved[3];
} sl2_sequence_blob_header;                    /* 256 bytes */
/* The layout arithmetic, host only (no device needed): offsets [capacity] receives off_x, off_P, off_slots, the
 * SL2_BLOB_SLOT_ARRAYS array offsets, off_seq, off_particles, off_traj, off_pos_log (SL2_BLOB_LAYOUT_OFFSETS values, as many as
 * fit); returns the blob's size in bytes, 0 for a negative argument. */
#define SL2_BLOB_LAYOUT_OFFSETS (7 + SL2_BLOB_SLOT_ARRAYS)
size_t sl2_sequence_blob_layout(int n_slots, int n_partial_slots, int n_particles, uint64_t* offsets, int capacity);
/* Upper bound of one blob of this engine (every slot, partial slot and particle in use), a multiple of 64. */
size_t sl2_sequence_blob_capacity(const sl2_engine* e);
/* One blob per sequence of [seq0, seq0 + nseq) at blobs + i * blob_stride (blob_stride >= sl2_sequence_blob_capacity, a multiple
 * of 64).  blobs_on_device != 0: one launch on the engine's stream, asynchronous, nothing else; `bytes` must be NULL (the size
 * is in each header).  Otherwise packed on the device into engine-owned staging of bounded size and copied out chunk by chunk,
 * one synchronisation per chunk; bytes [nseq] (may be NULL) receives each blob's size.  The engine is not changed. */
int sl2_save_sequences(sl2_engine* e, int seq0, int nseq, void* blobs, size_t blob_stride, int blobs_on_device, uint64_t* bytes);
/* The inverse, into sequences [seq0, seq0 + nseq).  blob_stride = distance between blobs AND the bytes available of each (any
 * multiple of 64 that holds the blob).  Every header is checked BEFORE anything is written (device blobs: the 256-byte headers
 * are fetched first): SL2_ERR_INVALID (magic, version, sizes, offsets, camera, params) or SL2_ERR_CAPACITY (the blob does not
 * fit this engine) with sl2_last_error() naming the field, and the engine untouched.  A blob with mapping in use switches
 * feature initialisation on (MatchPartiallyInitialisedFeatures goes on running, monoslam.cpp:167) and is refused with more
 * than one sequence group, like mapping itself.  Rows, columns and slots the blob does not cover are zeroed.  Synchronises;
 * captured step graphs are dropped.  The camera compared is the destination sequence's own (sl2_get_cameras), and a load never
 * changes it: give the slot the sequence's camera first (sl2_set_cameras). */
int sl2_load_sequences(sl2_engine* e, int seq0, int nseq, const void* blobs, size_t blob_stride, int blobs_on_device);
/* Save + load without the host, between two engines on one device or inside one engine (overlapping ranges: SL2_ERR_INVALID).
 * Engines on different streams are ordered by an event.  The destination is treated as by sl2_load_sequences, except that the two
 * engines' params.delta_t need not agree: the time step is the destination's own record (sl2_set_delta_t) and is not copied, so
 * engines created for cameras of different rates can hand sequences to each other.  The calibration is held to the same rule as
 * a load: source sequence i's camera must equal destination sequence i's. */
int sl2_copy_sequences(sl2_engine* dst, int dst_seq0, sl2_engine* src, int src_seq0, int nseq);
/* The sequences become what sl2_create left: empty map, next_free_label_ 0, counters, status, trajectory store, position log
 * and partial features cleared, drand48 as after srand48(0) (monoslam.cpp:1968), x and P zero.  The caller then sets the
 * vehicle state and adds features as for a fresh engine.  The sequence keeps its camera (sl2_set_cameras), its time step and
 * its place in the mask.  Synchronises; captured step graphs are dropped. */
int sl2_reset_sequences(sl2_engine* e, int seq0, int nseq);

/* ------------------------------------------------------------------- profiling */

/* enabled = 1: the roofline kernels (k_search_mfma, k_build_AS, k_chol_left, k_fwdsub_lds, k_syrk and their large-map
 * forms; narrowed by sl2_set_profile_focus) are bracketed by HIP events on the engine's stream; enabled = 2: every kernel
 * launch is; sl2_get_kernel_time returns accumulated milliseconds and launch counts per kernel symbol since the last reset. */
int sl2_set_profiling(sl2_engine* e, int enabled);
/* Level 1 brackets only the kernels named here (comma separated scope names, e.g. "k_syrk,k_search_mfma"; NULL or "" = the
 * four large ones): every bracket is two event markers on the stream, and four of them cost 1-3 % of a step. */
int sl2_set_profile_focus(sl2_engine* e, const char* names);
int sl2_reset_kernel_times(sl2_engine* e);
int sl2_kernel_count(sl2_engine* e);
int sl2_get_kernel_time(sl2_engine* e, int idx, const char** name, double* total_ms, int64_t* launches);
/* Algorithmic work of the last completed step summed over the batch:
 * out[0] = search window bytes sum_f (2hw+11)(2hh+11) capped per sequence at W*H,
 * out[1] = number of searched features, out[2] = in-ellipse candidates,
 * out[3] = sum over sequences of m (measurement rows), out[4] = sum of m^2,
 * out[5] = sum of m^3, out[6] = sum of n (state size) , out[7] = sum n*m, out[8] = sum n*n*m, out[9] = sum n*m*m,
 * out[10] = searches that took the exact fallback kernel path,
 * out[11] = 16 x 16 candidate tiles of the search windows, sum_f ceil(nu / 16) ceil(nv / 16): the matrix-core work of
 * k_search_mfma (24 v_mfma_i32_16x16x64_i8 per tile),
 * out[12] = search windows that were shared out over the wavefronts of the launch (sl2_set_search_split).
 * Sequences that are paused (sl2_set_active_sequences) when the call is made are left out of every sum. */
#define SL2_STEP_WORK_COUNT 13
/* capacity = length of the caller's array: min(capacity, SL2_STEP_WORK_COUNT) values are written (a caller built against a
 * header with fewer entries is never overrun; one built against more sees the extra entries untouched). */
int sl2_get_step_work(sl2_engine* e, double* out, int capacity);

/* How sl2_create placed the large matrices (an addition within SL2_API_VERSION 5).  The speed of the update's kernels depends on
 * the physical memory behind P, A^T, V^T and S - up to 8 % for k_build_AS at 1024 sequences x 100 features, fixed for the life of
 * an allocation, not visible in its address - so sl2_create times a streaming probe on several candidate allocations and keeps
 * the fastest of each kind (engines whose covariance is smaller than 256 MB: not tried, all zeros here).
 * out[0] = candidate allocations of P probed, out[1..4] = probe time in ms of the kept P, V^T, A^T, S, out[5..7] = of the slowest candidate
 * seen for P, for A^T / V^T, for S, out[8..9] = k_syrk itself on the kept pair (P, V^T) and on the slowest pair tried (the kernel
 * is its own probe: on an all-zero engine it does its full work and changes nothing).  min(capacity, SL2_PLACEMENT_COUNT) values
 * are written. */
#define SL2_PLACEMENT_COUNT 10
int sl2_get_placement(sl2_engine* e, double* out, int capacity);

/* ------------------------------------------------------------- synthetic input */

/* Render `count` frames of the synthetic textured plane z = 0:
 * poses [count][7] = camera r(3), q(w,x,y,z); tex = tex_size^2 8-bit texture
 * covering tex_extent metres (torus-wrapped), shifted by tex_origin[count][2].
 * out [count][height][width].  The device and host versions run the SAME source
 * (scenelib2_amd/csrc/sl2_synth.hpp) and produce identical bytes. */
int sl2_synth_render_host(const sl2_camera* cam, const uint8_t* tex, int tex_size, double tex_extent,
                          const double* tex_origin, const double* poses, int count, uint8_t* out);
int sl2_synth_render_device(int device, void* stream, const sl2_camera* cam, const uint8_t* tex_dev, int tex_size,
                            double tex_extent, const double* tex_origin_dev, const double* poses_dev, int count,
                            uint8_t* out_dev);

/* ------------------------------------------------------ device-memory helpers */
/* For hosts without their own HIP binding (the Python tests use these; a torch
 * caller passes tensor.data_ptr() instead). */
int sl2_dev_malloc(int device, size_t bytes, void** out);
int sl2_dev_free(int device, void* p);
int sl2_dev_upload(int device, void* dst_dev, const void* src_host, size_t bytes);
int sl2_dev_download(int device, void* dst_host, const void* src_dev, size_t bytes);

#ifdef __cplusplus
}
#endif
#endif /* SCENELIB2_AMD_H */
