/* scenelib2_amd_testing.h - TEST HOOKS AND MICRO-BENCHMARKS.  NOT part of the product ABI.
 *
 * These entry points exist only in scenelib2_amd/libscenelib2_amd_test.so (the same sources built with -DSL2_TESTING);
 * the product library libscenelib2_amd.so does not export them (tests/test_capi_symbols.py checks both).  The test
 * library is a full build: a hook that takes an engine works on an engine created by either library (same structures,
 * one shared HIP runtime).
 */
#ifndef SCENELIB2_AMD_TESTING_H
#define SCENELIB2_AMD_TESTING_H
#include "scenelib2_amd.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Feature::attempted_/successful_measurements_of_feature_ (feature.h:95-96) written directly: lets a test put a feature
 * in front of delete_bad_features without ten frames of failed matches.  Synchronises. */
int sl2_set_feature_counters(sl2_engine* e, int seq, int label, int attempted, int successful);

/* The error of a feature's recorded position_in_total_state_vector_ (how far it lies below the true one: a multiple of three,
 * what feature.cpp:254 - Q28 - accumulates over conversions), written directly.  Lets a test drive the dh_by_dy block of H into
 * the vehicle state (monoslam.cpp:562-565: it OVERWRITES dh_by_dxv there) and below column 0
 * (SL2_STATUS_REFERENCE_OUT_OF_BOUNDS) without the dozen conversions that would take.  Synchronises. */
int sl2_debug_set_position_error(sl2_engine* e, int seq, int label, int err);

/* How many steps this engine has captured into graphs since sl2_create (sl2_set_graph_mode): a step that is replayed does not
 * count, one that had to be captured again - because a setter dropped the graphs, or the step's key changed - does. */
int sl2_debug_graph_captures(sl2_engine* e);

/* The plan launch_update would make now for sequence group `group` of the engine (csrc/sl2_update_plan.hpp: make_update_plan on
 * the group's shape and the engine's knobs), as update_plan_ints lays it out: build form, threads, nsplit, LDS bytes; Cholesky
 * form, panel blocks; substitution form, nb, group rows.  n: ints of room in out, at least 9.  Host arithmetic only.  (The plan is this library's: for an engine of
 * the product library it differs where a step has no product form - which no engine the product library creates reaches.) */
int sl2_debug_update_plan(sl2_engine* e, int group, int* out, int n);

/* The covariance of one sequence as the kernels hold it: P [ld][ld] with ld = *ld (the state columns rounded up to 64), the
 * padding rows and columns and the columns of never-used slots included - what sl2_get_total_covariance leaves out.
 * capacity_ld: rows and columns of room in P; too few: SL2_ERR_CAPACITY with *ld set.  Synchronises. */
int sl2_debug_raw_covariance(sl2_engine* e, int seq, double* P, int capacity_ld, int* ld);

/* FP64 epilogue of correlate2_warning (improc.cpp:99-133) evaluated ON THE DEVICE
 * for `count` tuples of the five integer sums: checks IEEE div/sqrt parity. */
int sl2_debug_ncc_score(int device, const int32_t* sums5, int count, double* score, double* sd0, double* sd1);
/* C[M][N] = sum_k XT[k][m] * YT[k][n] on the FP64 MFMA tile path used by the EKF
 * kernels (k-major operands): XT [K][ldx], YT [K][ldy], C [M][ldc].  Host pointers. */
int sl2_debug_gemm_kt(int device, const double* XT, int ldx, const double* YT, int ldy, int M, int N, int K,
                      double* C, int ldc);

/* Micro-benchmarks that calibrate the roofline peaks on the box: which = 0 FP64 MFMA
 * TFLOP/s (4 independent accumulators), 1 = dependent chain, 2 = streaming copy GB/s. */
int sl2_debug_microbench(int device, int which, double* result);

/* Rows of a frame one workgroup of k_frame_stats covers (kFrameBandRows of scenelib2_amd/csrc/sl2_frame_monitor_dev.hpp, which
 * sl2_frame_monitor.hip checks against this): the tests put image heights one row before, at and one row after a band's end. */
#define SL2_FRAME_MONITOR_BAND_ROWS 32

#ifdef __cplusplus
}
#endif
#endif /* SCENELIB2_AMD_TESTING_H */
