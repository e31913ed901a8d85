// What one sl2_go_one_step launches, decided ONCE: the step plan.  sl2_go_one_step makes it, its launch list walks it, the
// launchers take their per-step arguments from it, and a captured step (HIP graph) is keyed by it - so a choice that a capture
// bakes in cannot be missing from the key: a launcher has nothing else to decide from.
// Host-only arithmetic, no HIP: tests/step_plan_host.cpp compiles this header alone.
#pragma once

namespace sl2 {

constexpr int kSmallM = 32;          // rows of the innovation system of the fused small-map update (one Cholesky block)
constexpr int kSmallW = 128;         // compact columns at most: 13 + 3 * 36 + 6 + 1
constexpr int kSmallBatchMax = 256;  // sequences per group up to which the fused step is the faster one at ANY capacity (scripts/small_latency.py)

// One sequence group's part of the step.
struct GroupPlan {
  bool small_front = false;  // k_small_front in place of predict + feature prediction + select
  bool small_back = false;   // k_small_back (behind the search kernel alone) in place of score + update + finalize
  int panel_w = 0;           // columns of k_small_back's LDS panel: 64 or kSmallW; 0 = the back is not fused
  int save_trajectory = 0;   // what the group's finalize / k_small_back receives: with the tail the push moves behind it (k_map_update)
  bool operator==(const GroupPlan& o) const {
    return small_front == o.small_front && small_back == o.small_back && panel_w == o.panel_w && save_trajectory == o.save_trajectory;
  }
};

// The feature-initialisation tail (sl2_mapping.hip: launch_mapping).  A flag is set only when the launch is made; without the
// tail every member is zero.
struct TailPlan {
  bool runs = false;         // once mapping has been on, MatchPartiallyInitialisedFeatures has work in every later step (monoslam.cpp:167 is unconditional)
  int enable_mapping = 0;
  int save_trajectory = 0;
  bool squeeze = false;      // k_map_compact_slots
  bool find = false;         // k_map_find
  bool create = false;       // k_map_create
  bool partials = false;     // k_map_particles, k_map_me_search, k_me_big, k_map_update
  bool finish = false;       // k_map_finish in place of create + update
  int parts_full = 0;        // k_map_particles' argument: it clears the two per-step flags k_map_find would have
  bool operator==(const TailPlan& o) const {
    return runs == o.runs && enable_mapping == o.enable_mapping && save_trajectory == o.save_trajectory && squeeze == o.squeeze &&
           find == o.find && create == o.create && partials == o.partials && finish == o.finish && parts_full == o.parts_full;
  }
};

// group_range (sl2_seq_arrays.hpp) hands out at most two distinct group sizes: [0] is the plan of the longer groups (the first
// B % G), [1] of the others (the same plan where all groups are of one size).
struct StepPlan {
  GroupPlan group[2];
  TailPlan tail;
  bool operator==(const StepPlan& o) const { return group[0] == o.group[0] && group[1] == o.group[1] && tail == o.tail; }
};

// The engine's static shape and knobs, as far as a plan depends on them.
struct StepShape {
  int N, ld, mld, kpart;     // sl2_engine's members of these names
  int step_fusion;           // sl2_set_step_fusion: 0 = never fused, 1 = the rule below, 2 = both sides fused whatever the batch
  bool mapping_used;         // feature initialisation is in use (enable_mapping once, or an "initialise feature" call)
  int group_B[2];            // sequences of a longer and of a shorter group (equal with one group or B % G == 0)
};

// Which stages of a sequence group's step are fused: 0 = none (ten launches), 1 = both sides of the search (three launches),
// 2 = the back side only (scoring + update + finalize in one launch, the front-end stages on their own: six launches).
// Static conditions: at most 16 features measured per frame - the innovation system is one 32 x 32 block - and one partially
// initialised feature in flight at most (a misplaced recorded position, Q28, is taken from f_hcol like the ten-launch step
// does; the host cannot know of one without a synchronisation, so it is not a condition).  Dynamic: the LIVE maps fit
// kSmallW columns - `slots_bound` = the host's upper bound on n_slots of any sequence (sl2_engine.hip: slots_upper_bound, exact
// at synchronised points, from the device's mailbox in between).  Then: everything fused when the group is small enough to be
// latency-bound or the capacity is large (the one-stage kernels work on all ld columns, the fused ones on the live ones:
// scripts/small_latency.py, a dozen features at capacity 128 - ld = 448 - fused is 1.2 x faster at one sequence and 1.8 x at
// 1024); at a small capacity and a large batch only the back side, which holds its own there (0.107 against 0.118 ms for the six
// stages it replaces at 1024 sequences, ld = 128) - k_small_front does not (0.065 against 0.038 ms: 304 registers, one workgroup
// per CU).
inline int small_step_mode(const StepShape& s, int group_B, int slots_bound) {
  if (!s.step_fusion || s.mld != kSmallM || s.kpart != 1 || 13 + 3 * slots_bound + 6 * s.kpart + 1 > kSmallW) return 0;
  return (group_B <= kSmallBatchMax || s.ld >= 256 || s.step_fusion == 2) ? 1 : 2;
}

// Columns of k_small_back's LDS panel for a group whose live maps are at most `slots_bound` slots: 64 while every map fits
// them (a third workgroup per CU at large batches), else kSmallW.  The kernel picks its own W from each sequence's size, which
// the bound bounds; a captured step bakes this choice in.
inline int small_panel_w(const StepShape& s, int slots_bound) {
  return (13 + 3 * slots_bound + 6 * s.kpart + 1 <= 64) ? 64 : kSmallW;
}

// The plan of the step about to be issued.  slots_bound: sl2_engine.hip: slots_upper_bound.  parts_state: what the host knows
// about the partially initialised features the step starts with (sl2_engine.hip: parts_state_for_step) - 1 = none, 2 = every
// partial slot taken, 0 = not known: every launch of the tail.
inline StepPlan make_step_plan(const StepShape& s, int slots_bound, int parts_state, int save_trajectory, int enable_mapping) {
  StepPlan p;
  for (int k = 0; k < 2; ++k) {
    const int mode = small_step_mode(s, s.group_B[k], slots_bound);
    GroupPlan& g = p.group[k];
    g.small_front = mode == 1;
    g.small_back = mode != 0;
    g.panel_w = mode != 0 ? small_panel_w(s, slots_bound) : 0;
    g.save_trajectory = s.mapping_used ? 0 : save_trajectory;
  }
  if (!s.mapping_used) return p;
  TailPlan& t = p.tail;
  t.runs = true;
  t.enable_mapping = enable_mapping ? 1 : 0;
  t.save_trajectory = save_trajectory;
  // Retired slots are squeezed out only when a sequence is about to run out of slots; the bound says when none can be: the
  // launch - one of the step's dependent chain, 7 us at one sequence, 0.03 ms at 1024 - is then left out altogether.
  t.squeeze = enable_mapping && slots_bound + 1 > s.N;
  // The three launches that serve partially initialised features are dead weight while there is none, and at one sequence each
  // is a link of the frame's dependent chain: k_map_update's report lets the host leave them out (state 1), creation and
  // bookkeeping then being one launch.  me_big_count keeps its last value meanwhile; k_map_particles zeroes it before anything
  // reads it again.  The other way round (state 2): every partial slot is taken, so FindNonOverlappingRegion's gate (k_map_find:
  // kPartCount < kpart, monoslam.cpp:163-165) is shut whatever the camera does - no region, no detector, no creation.
  const bool parts_none = parts_state == 1, parts_full = parts_state == 2;
  t.find = !parts_full;
  t.finish = parts_none;
  t.create = !parts_full && !parts_none;
  t.partials = !parts_none;
  t.parts_full = parts_full ? 1 : 0;
  return p;
}

}  // namespace sl2
