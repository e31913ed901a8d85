// Host build of the step plan (sl2_step_plan.hpp, no HIP): what tests/test_step_plan_host.py asks of it.
#include "../scenelib2_amd/csrc/sl2_step_plan.hpp"

using namespace sl2;

namespace {
// in: N, ld, mld, kpart, step_fusion, mapping_used, sequences of a longer group, of a shorter group, slots_bound, parts_state,
// save_trajectory, enable_mapping
constexpr int kIn = 12;
// out: per group (longer, shorter) small_front, small_back, panel_w, save_trajectory; then the tail's runs, enable_mapping,
// save_trajectory, squeeze, find, create, partials, finish, parts_full
constexpr int kOut = 17;

StepPlan plan_of(const int* in) {
  const StepShape s = {in[0], in[1], in[2], in[3], in[4], in[5] != 0, {in[6], in[7]}};
  return make_step_plan(s, in[8], in[9], in[10], in[11]);
}
}  // namespace

extern "C" {

int sp_in_ints() { return kIn; }
int sp_out_ints() { return kOut; }
int sp_constant(int which) { return which == 0 ? kSmallM : which == 1 ? kSmallW : which == 2 ? kSmallBatchMax : -1; }

// the plans of n inputs, member by member
void sp_plans(const int* in, int n, int* out) {
  for (int i = 0; i < n; ++i, in += kIn, out += kOut) {
    const StepPlan p = plan_of(in);
    int* o = out;
    for (const GroupPlan& g : p.group) { *o++ = g.small_front; *o++ = g.small_back; *o++ = g.panel_w; *o++ = g.save_trajectory; }
    const TailPlan& t = p.tail;
    *o++ = t.runs; *o++ = t.enable_mapping; *o++ = t.save_trajectory; *o++ = t.squeeze; *o++ = t.find; *o++ = t.create;
    *o++ = t.partials; *o++ = t.finish; *o++ = t.parts_full;
  }
}

// operator== between the plan of input i and the plan of input ref[i]
void sp_equal(const int* in, int n, const int* ref, int* out) {
  for (int i = 0; i < n; ++i) out[i] = plan_of(in + (long)i * kIn) == plan_of(in + (long)ref[i] * kIn) ? 1 : 0;
}

}  // extern "C"
