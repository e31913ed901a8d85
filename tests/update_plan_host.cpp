// Host build of the update plan (sl2_update_plan.hpp, no HIP): what tests/test_update_plan_host.py asks of it.
#include "../scenelib2_amd/csrc/sl2_update_plan.hpp"

using namespace sl2;

namespace {
// in: max_features, number_of_features_to_select, kpart, group_from, panel_from (update_sizes); the group's sequences; then
// build_variant, chol_variant, fwd_variant, build_split, build_ahead, build_lds_min, no_ksplit, fwd_group, chol_panel, superseded
constexpr int kIn = 16;
// out: ld, ppos, nsel_max, mld, nblk_max, update_sizes_admitted; the plan (update_plan_ints); which text error() gives (0: none)
constexpr int kOut = 6 + kUpdatePlanInts + 1;

UpdateSizes sizes_of(const int* in) { return update_sizes(in[0], in[1], in[2], in[3], in[4]); }

UpdatePlan plan_of(const int* in) {
  const UpdateSizes z = sizes_of(in);
  const UpdateShape s = {in[5], in[0], z.ld, z.mld, z.nblk_max, z.nsel_max, in[6], in[7], in[8], in[9], in[10], in[11], in[12],
                         in[4], in[3], in[13], in[14], in[15] != 0};
  return make_update_plan(s);
}

// the two plans error() can speak of: the texts themselves go out through up_error_text
UpdatePlan plan_without(int which) {
  UpdatePlan p;
  p.chol = which == 1 ? CholForm::kNone : CholForm::kLeft;
  p.fwd = which == 2 ? FwdForm::kNone : FwdForm::kKsplit;
  return p;
}
}  // namespace

extern "C" {

int up_in_ints() { return kIn; }
int up_out_ints() { return kOut; }
int up_constant(int which) {
  const int c[] = {kASBatch, kAheadEntry, kAheadLdsMax, kBuildOneThreadLd, kBuildFullBatch, kBuildWorkgroups, kKsMaxBlocks,
                   kKsMaxStrips, kFwdLdsMaxBlocks, kCholPanelBlocks, kUpdateLdMax, kUpdateMldMax};
  return which >= 0 && which < (int)(sizeof(c) / sizeof(c[0])) ? c[which] : -1;
}
const char* up_error_text(int which) { return plan_without(which).error(); }

// the sizes and the plans of n inputs, member by member
void up_plans(const int* in, int n, int* out) {
  for (int i = 0; i < n; ++i, in += kIn, out += kOut) {
    const UpdateSizes z = sizes_of(in);
    const UpdatePlan p = plan_of(in);
    out[0] = z.ld; out[1] = z.ppos; out[2] = z.nsel_max; out[3] = z.mld; out[4] = z.nblk_max; out[5] = update_sizes_admitted(z);
    update_plan_ints(p, out + 6);
    const char* err = p.error();
    out[6 + kUpdatePlanInts] = !err ? 0 : err == plan_without(1).error() ? 1 : err == plan_without(2).error() ? 2 : -1;
  }
}

// operator== between the plan of input i and the plan of input ref[i]
void up_equal(const int* in, int n, const int* ref, int* out) {
  for (int i = 0; i < n; ++i) out[i] = plan_of(in + (long)i * kIn) == plan_of(in + (long)ref[i] * kIn) ? 1 : 0;
}

}  // extern "C"
