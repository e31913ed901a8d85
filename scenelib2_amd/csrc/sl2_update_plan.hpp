// What the dense EKF update (launch_update, sl2_ekf_update.hip, and the phase units sl2_update_*.hip) launches, decided ONCE: the sizes sl2_create gives the innovation system, and the
// update plan - the form of every step of the update (build A and S, factor S, substitute; the SYRK has one form) with the launch
// parameters that depend on the shape.  launch_update makes the plan per call from the engine's shape and knobs and walks it;
// the launchers take their widths from it and compare nothing themselves.
// Host-only arithmetic, no HIP: tests/update_plan_host.cpp compiles this header alone.
#pragma once

namespace sl2 {

inline int round_up(int v, int a) { return (v + a - 1) / a * a; }

// ---- the constants the choices rest on (the kernels use them by name)
constexpr int kASBatch = 4;            // k_build_AS: features per LDS batch (state sizes up to 1024 columns)
constexpr int kAheadEntry = 24;        // k_build_AS_ahead: doubles per entry of the measurement table: Hx 0..13, Hy 14..19, nu 20..21, R 22, pos 23 (an integer)
constexpr int kAheadLdsMax = 40960;    // bytes of LDS per workgroup the form may take (a quarter of the CU's 160 KB)
constexpr int kBuildOneThreadLd = 1024;   // state columns up to which a k_build_AS thread owns ONE column (beyond: two, of a 1024-thread workgroup); also the largest ld of k_build_AS_ahead
// k_build_AS: one workgroup per sequence from batch kBuildFullBatch on (one exact round of four per CU at 1024; it needs the launch
// in front of it - k_search_score - to consist of single-wave workgroups, see launch_search).  Smaller batches: ~kBuildWorkgroups
// workgroups in all, so that the chip is full and a sequence's 25 feature batches are not one chain.
constexpr int kBuildFullBatch = 1024;
constexpr int kBuildWorkgroups = 3072;
constexpr int kKsMaxBlocks = 8;        // k_fwdsub_ksplit: 32-blocks at most (its solved block rows live in LDS) ...
constexpr int kKsMaxStrips = 160;      // ... and 16-column strips in the launch at most: small batches, where k_fwdsub_lds is a chain
constexpr int kFwdLdsMaxBlocks = 13;   // k_fwdsub_lds<NB>: the register-resident strip of solved block rows, NB = 1 .. 13
constexpr int kCholPanelBlocks = 4;    // 32-blocks per panel of the panel-wise Cholesky (or 8: sl2_engine::chol_panel); nblk_max is a multiple of it there
// What sl2_create admits (product build): k_build_AS gives two state columns to each thread of a 1024-thread workgroup, one H row per thread
constexpr int kUpdateLdMax = 2048;     // state columns: 676 feature slots
constexpr int kUpdateMldMax = 1024;    // rows of the innovation system: 512 features measured per frame

// ---- the sizes (sl2_create)
struct UpdateSizes {
  int ld;        // leading dimension of x / P / At / Vt rows: xv(13), 3 per feature slot, 6 per partially initialised feature in
                 // flight (kpart of them), 1 for the innovation (At / Vt), rounded up to 64
  int ppos;      // first column of the partial features' states
  int nsel_max;  // features measured per frame at most: number_of_features_to_select, within 1 .. max_features
  int mld;       // leading dimension of the innovation system: 2 nsel_max rounded up to 32; to 64 beyond the one-launch
                 // substitution (group_from blocks: 64-row tiles, k_fwd_gemm); to 128 where it is factored in panels (panel_from)
  int nblk_max;  // mld / 32
};

inline UpdateSizes update_sizes(int max_features, int number_of_features_to_select, int kpart, int group_from, int panel_from) {
  UpdateSizes s;
  s.ld = round_up(13 + 3 * max_features + 6 * kpart + 1, 64);
  s.ppos = 13 + 3 * max_features;
  int nsel = number_of_features_to_select;
  if (nsel < 1) nsel = 1;
  if (nsel > max_features) nsel = max_features;
  s.nsel_max = nsel;
  s.mld = round_up(2 * nsel, 32);
  if (s.mld / 32 > group_from) s.mld = round_up(2 * nsel, 64);
  if (s.mld / 32 > panel_from) s.mld = round_up(2 * nsel, 128);
  s.nblk_max = s.mld / 32;
  return s;
}

// the product library creates no engine beyond these (the TEST build does: its superseded kernels take any size)
inline bool update_sizes_admitted(const UpdateSizes& s) { return s.ld <= kUpdateLdMax && s.mld <= kUpdateMldMax; }

// ---- the plan
enum class BuildForm : int { kTwoPass, kAS14, kAS22, kAhead4, kAhead2 };     // k_build_A + k_build_S (superseded) | k_build_AS<1,4> | <2,2> | k_build_AS_ahead<4> | <2>
enum class CholForm : int { kNone, kLeft, kPanels, kPerBlock };              // k_chol_left | launch_chol_panels | three launches per block column (superseded)
enum class FwdForm : int { kNone, kKsplit, kLds, kGrouped, kReread };        // k_fwdsub_ksplit | k_fwdsub_lds<NB> | launch_fwdsub_grouped | k_fwdsub (superseded)

// A sequence group's shape and the root engine's knobs, as far as the plan depends on them (sl2_engine's members of these names).
struct UpdateShape {
  int B, N, ld, mld, nblk_max, nsel_max;
  int build_variant, chol_variant, fwd_variant;
  int build_split, build_ahead, build_lds_min, no_ksplit;
  int panel_from, group_from, fwd_group, chol_panel;
  bool superseded;          // the superseded kernels exist: the TEST build of the library
};

struct UpdatePlan {
  BuildForm build = BuildForm::kAS14;
  int build_threads = 0;    // workgroup size (kTwoPass: k_build_A's; k_build_S has its own)
  int build_nsplit = 1;     // workgroups per sequence: ranges of feature batches
  int build_lds_bytes = 0;  // dynamic LDS per workgroup
  CholForm chol = CholForm::kNone;
  int chol_panel_blocks = 0;   // kPanels: 32-blocks per panel, 4 or 8
  FwdForm fwd = FwdForm::kNone;
  int fwd_nb = 0;           // kLds: the instantiation, 1 .. kFwdLdsMaxBlocks
  int fwd_group_rows = 0;   // kGrouped: block rows per group, 4 or 8
  bool operator==(const UpdatePlan& o) const {
    return build == o.build && build_threads == o.build_threads && build_nsplit == o.build_nsplit &&
           build_lds_bytes == o.build_lds_bytes && chol == o.chol && chol_panel_blocks == o.chol_panel_blocks && fwd == o.fwd &&
           fwd_nb == o.fwd_nb && fwd_group_rows == o.fwd_group_rows;
  }
  // why launch_update refuses, where a step has no form (the factorisation is met first); nullptr: every step has one
  const char* error() const {
    if (chol == CholForm::kNone) return "launch_update: no factorisation for this system size (sl2_create should have padded it)";
    if (fwd == FwdForm::kNone) return "launch_update: no substitution kernel for this system size (sl2_create should have padded it)";
    return nullptr;
  }
};

inline UpdatePlan make_update_plan(const UpdateShape& s) {
  UpdatePlan p;
  // ---- A = P H^T and S = H A + R
  if (s.build_variant == 0 && s.superseded) {
    p.build = BuildForm::kTwoPass;
    p.build_threads = s.ld <= 512 ? s.ld : 512;
  } else {
    int nsplit = s.B >= kBuildFullBatch ? 1 : (kBuildWorkgroups + s.B - 1) / s.B;
    if (s.build_split > 0) nsplit = s.build_split;        // experiments (TEST build: SL2_BUILD_SPLIT)
    if (nsplit < 1) nsplit = 1;
    const int nbatch_max = (s.N + kASBatch - 1) / kASBatch;      // (from the capacity, for every form)
    if (nsplit > nbatch_max) nsplit = nbatch_max;
    // One workgroup per sequence, ld <= 1024: the form that keeps a batch of rows in flight (k_build_AS_ahead), with four
    // features per batch where its LDS (the batch's rows of At + the measurement table of nsel_max entries) stays inside
    // kAheadLdsMax, else two; where neither does (large maps that also measure many features per frame), k_build_AS.
    int ahead = 0;
    if (nsplit == 1 && s.ld <= kBuildOneThreadLd && s.build_ahead != 0)
      for (int batch = 4; batch >= 2 && !ahead; batch -= 2)
        if (8 * (2 * batch * s.ld + kAheadEntry * s.nsel_max) <= kAheadLdsMax) ahead = batch;
    p.build_nsplit = nsplit;
    if (ahead) {
      p.build = ahead == 4 ? BuildForm::kAhead4 : BuildForm::kAhead2;
      p.build_threads = s.ld;
      p.build_lds_bytes = 8 * (2 * ahead * s.ld + kAheadEntry * s.nsel_max);
    } else if (s.ld <= kBuildOneThreadLd) {
      p.build = BuildForm::kAS14;
      p.build_threads = s.ld;
      p.build_lds_bytes = 8 * 2 * kASBatch * s.ld;
    } else {
      p.build = BuildForm::kAS22;
      p.build_threads = 1024;
      p.build_lds_bytes = 8 * 2 * 2 * s.ld;      // <= 64 KB
    }
    // (TEST build: SL2_BUILD_LDS_MIN caps the workgroups a CU takes)
    if (p.build != BuildForm::kAS22 && s.build_lds_min > p.build_lds_bytes) p.build_lds_bytes = s.build_lds_min;
  }
  // ---- S = L L^T.  sl2_create sizes the innovation system so that one of the first two always applies (mld a multiple of 128
  // beyond 16 blocks)
  if (s.nblk_max > s.panel_from && s.chol_variant >= 1 && s.mld % 64 == 0 && s.nblk_max % kCholPanelBlocks == 0) {
    p.chol = CholForm::kPanels;
    // panel width in 32-blocks: 4 (128 columns) or 8 (256 columns: half as many trailing updates, each with twice the K)
    p.chol_panel_blocks = s.chol_panel == 8 ? 8 : kCholPanelBlocks;
  } else if (s.nblk_max <= s.panel_from && s.chol_variant == 1) {
    p.chol = CholForm::kLeft;
  } else if (s.superseded) {
    p.chol = CholForm::kPerBlock;
  }
  // ---- V = A L^-T
  if (s.fwd_variant == 1) {
    if (s.nblk_max <= kKsMaxBlocks && (long long)s.B * (s.ld / 16) <= kKsMaxStrips && !s.no_ksplit) {
      p.fwd = FwdForm::kKsplit;      // small batches: the chain-shortening kernel (one 16-column strip per workgroup)
    } else if (s.nblk_max <= s.group_from && s.nblk_max <= kFwdLdsMaxBlocks) {
      p.fwd = FwdForm::kLds;
      p.fwd_nb = s.nblk_max;
    } else if (s.mld % 64 == 0) {
      // beyond the register-resident strip: groups of eight (or four: fwd_group) block rows on 64-row tiles (sl2_create pads
      // systems of more than group_from blocks to 64, of more than panel_from to 128)
      p.fwd = FwdForm::kGrouped;
      p.fwd_group_rows = s.fwd_group == 4 ? 4 : 8;
    }
  }
  if (p.fwd == FwdForm::kNone && s.superseded) p.fwd = FwdForm::kReread;
  return p;
}

// The plan as a record of ints, in the order of its members (the TEST build's sl2_debug_update_plan, tests/update_plan_host.cpp).
constexpr int kUpdatePlanInts = 9;
inline void update_plan_ints(const UpdatePlan& p, int* out) {
  out[0] = (int)p.build; out[1] = p.build_threads; out[2] = p.build_nsplit; out[3] = p.build_lds_bytes;
  out[4] = (int)p.chol; out[5] = p.chol_panel_blocks;
  out[6] = (int)p.fwd; out[7] = p.fwd_nb; out[8] = p.fwd_group_rows;
}

}  // namespace sl2
