// EKF update — Kalman::KalmanFilterUpdate (kalman.cpp:72-119) for the whole batch.
//
// Reference algebra:  S = H P H^T + R ; W = P H^T S^-1 ; x += W nu ; P -= W S W^T.
// Executed here as (mathematically identical, FP64 throughout):
//   A  = P H^T                     sparse rows of H: 7 pose + 3 feature columns (a6/a14)      sl2_update_build.hip
//   S  = H A + R = L L^T           blocked Cholesky, 32x32 blocks                             sl2_update_chol.hip
//   V  = A L^-T                    blocked forward substitution (one pass over A)             sl2_update_fwdsub.hip
//   P -= V V^T ; x += V (L^-1 nu)  SYRK; nu rides along as an extra column of A               sl2_update_syrk.hip
// because W S W^T = A S^-1 A^T = V V^T and W nu = V L^-1 nu.
//
// All dense operands are stored "k-major" (XT[k][i]: the contraction index is the
// slow one) so that every FP64 MFMA fragment (v_mfma_f64_16x16x4_f64: A[i=l&15]
// [k=l>>4], B[k=l>>4][j=l&15], D[row=(l>>4)+4r][col=l&15]) is a 128-byte
// coalesced row segment per 16 lanes, and the D fragment of one product is
// directly the B fragment (k-step s == register s) of the next.
//
// This unit is the walk over the plan; each phase's kernels and launcher are a translation unit of their own, compiled once and
// linked into both libraries.  The superseded kernels and the test / calibration entry points are sl2_update_testing.hip, in
// the TEST library alone: this unit is built a second time with -DSL2_TESTING for it, so that the plan may name their forms.
#include "sl2_common.hpp"

namespace sl2 {

#ifdef SL2_TESTING
constexpr bool kSupersededKernels = true;
#else
constexpr bool kSupersededKernels = false;
#endif  // SL2_TESTING

// What make_update_plan takes: the shape of the engine (a sequence group) and the knobs of its root.
UpdateShape update_shape(const sl2_engine* e) {
  const sl2_engine* r = e->root;
  return {e->B, e->N, e->ld, e->mld, e->nblk_max, e->nsel_max, r->build_variant, r->chol_variant, r->fwd_variant,
          r->build_split, r->build_ahead, r->build_lds_min, r->no_ksplit, r->panel_from, r->group_from, r->fwd_group,
          r->chol_panel, kSupersededKernels};
}

// The update of one sequence group, as its plan says (sl2_update_plan.hpp): build A and S, factor S, substitute, SYRK.  The
// plan is made per call - a few dozen integer operations - so there is no copy to go stale when a knob changes.
// Profiling scopes carry the SYMBOL of the kernel they bracket (so that the bench's per-kernel times and rocprofv3's
// kernel_stats.csv join on the name); "@phase" tells two uses of one kernel apart (k_fwdsub_lds is also the panel solve of
// the large-map Cholesky).
// Every kernel of the update takes its row count from a pointer and leaves at once on 0 - before it writes anything to x or P
// (At / Vt / St / LinvT are rebuilt by every update).  What they are handed is m_gate: m_count for a sequence that takes part in
// the step, 0 for a paused one (k_search_score; sl2_set_active_sequences), so a paused sequence costs these kernels one load.
// (succ_idx / m_count, the successful measurements in slot order, come from k_search_score.)
int launch_update(sl2_engine* e) {
  const UpdatePlan p = make_update_plan(update_shape(e));
  // a step in a form the product has no kernel for: its superseded launcher (TEST build), else the plan's refusal
  enum { kBuild, kFactor, kSubstitute };
  auto other_form = [&](int step) -> int {
#ifdef SL2_TESTING
    switch (step) {
      case kBuild: if (p.build == BuildForm::kTwoPass) return launch_build_two_pass(e, p.build_threads); break;
      case kFactor: if (p.chol == CholForm::kPerBlock) return launch_chol_per_block(e); break;
      case kSubstitute: if (p.fwd == FwdForm::kReread) return launch_fwdsub_reread(e); break;
    }
#else
    (void)step;
#endif
    set_error(p.error() ? p.error() : "launch_update: the plan names a kernel this library does not have");
    return SL2_ERR_INVALID;
  };
  // ---- A = P H^T, S = H A + R
  int rc = launch_build(e, p);
  if (rc == kNoProductForm) rc = other_form(kBuild);
  if (rc != SL2_OK) return rc;
  // ---- S = L L^T
  rc = launch_factor(e, p);
  if (rc == kNoProductForm) rc = other_form(kFactor);
  if (rc != SL2_OK) return rc;
  // ---- V = A L^-T
  rc = launch_substitute(e, p);
  if (rc == kNoProductForm) rc = other_form(kSubstitute);
  if (rc != SL2_OK) return rc;
  // ---- P -= V V^T, x += V (L^-1 nu)
  return launch_product(e);
}

}  // namespace sl2
