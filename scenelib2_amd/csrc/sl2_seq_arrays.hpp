// The engine's per-sequence device arrays, listed ONCE: every array of shape [B][something] is one row of SL2_SEQ_ARRAYS.
// The members of the engine object, their allocation (sl2_create), a sequence group's view of them (build_groups) and their
// release (sl2_destroy) are all expansions of that list, so an array cannot be missing from one of them or carry two extents.
// Host-only arithmetic, no HIP: tests/seq_arrays_host.cpp compiles this header alone.
#pragma once
#include <cstddef>
#include <cstdint>

namespace sl2 {

// ---- layout constants the extents are written in ----
constexpr int kTrajCapacity = 1000;  // monoslam.cpp:174
constexpr int kParticleDoubles = 12; // lambda, probability, cumulative, h[2], z[2], SInv(00,01,11), detS, success
constexpr int kPartInts = 16, kPartDoubles = 4;   // part_i / part_d, the per-SEQUENCE record of the partially initialised features (fields: sl2_common.hpp)
constexpr int kPsInts = 8, kPsDoubles = 4;        // ps_i / ps_d, one record per PARTIAL SLOT; ps_d: mean, covariance of lambda
constexpr int kWorkDoubles = 5;      // per-sequence work counters of a step (work[]): window bytes, searches, candidates, exact
                                     // fallbacks, 16 x 16 candidate tiles of the matrix-core search
constexpr int kSeqTimeDoubles = 4;   // seq_time, the per-sequence time record (the places of its fields: sl2_common.hpp)
constexpr int kSeqCamDoubles = 8;    // seq_cam, the per-sequence camera calibration: one 64-byte line (fields: sl2_common.hpp)
constexpr int kPatchStride = 288;    // bytes per stored template: 121 raw bytes (+7 pad), then at byte
                                     // 128 the packed form: 33 dwords (11 rows x 12 bytes, byte 11 = 0),
                                     // sum g0, sum g0^2, flag (patch sigma >= 10), pad

// What the extents depend on, and nothing else (sl2_engine carries the same values as ints).
struct SeqDims {
  size_t N;         // feature capacity per sequence
  size_t ld;        // leading dimension of x / P / At / Vt rows
  size_t mld;       // leading dimension of the innovation system
  size_t nblk_max;  // mld / 32
  size_t kpart;     // partial slots per sequence
  size_t pcap;      // particle slots per partial feature
};

// X(type, name, elements per sequence): the array is type name[B][elements], rows in the order sl2_create allocates them
// (where the large matrices land decides the speed of k_build_AS and k_syrk - sl2_engine.hip: place_large_matrices - so the
// order is part of what a timing compares).  The third column is an expression over the members of SeqDims and the
// constants above.  Each row's comment says what the inner indices are.
#define SL2_SEQ_ARRAYS(X)                                                                                                          \
  /* ---- persistent SLAM state ---- */                                                                                            \
  X(double, x, ld)                        /* [ld]        total state: xv(13), y_0(3), y_1(3) ... ; x[ld-1] unused */                \
  X(double, P, ld * ld)                   /* [ld][ld]    total covariance, dense; row/col ld-1 always zero */                        \
  X(uint8_t, patch, N * kPatchStride)     /* [N][kPatchStride]  11x11 templates, raw and packed (kPatchStride above) */              \
  X(int, patch_sums, N * 2)               /* [N][2]      (sum g0, sum g0^2) of each template */                                      \
  X(double, xp_org, N * 8)                /* [N][8]      xp_org_ (7 used) */                                                         \
  X(int, f_flags, N)                      /* [N]         FF_* bits (sl2_common.hpp) */                                               \
  X(int, n_slots, 1)                      /*             slots in use (live, reserved or retired features), list order = slot order */ \
  X(int, f_label, N)                      /* [N]         Feature::label_ of the slot (slots are compacted when they run out, labels never reused) */ \
  X(int, next_label, 1)                   /*             next_free_label_ */                                                         \
  X(int, attempted, N)                    /* [N] */                                                                                  \
  X(int, successful, N)                   /* [N] */                                                                                  \
  X(double, traj, kTrajCapacity * 3)      /* [kTrajCapacity][3] */                                                                   \
  X(int, traj_count, 1)                   /*             total pushes */                                                             \
  X(double, last_r, 3)                    /* [3]         scratch motion_model_->rRES_ (Q12) */                                       \
  X(int, status, 1)                                                                                                                \
  X(double, pos_log, kTrajCapacity * 3)   /* [kTrajCapacity][3] xv[0:3] after every step (the true trajectory, cf. Q12) */           \
  X(int, pos_count, 1)                    /*             steps logged so far (device-side, so that a captured step needs no per-step argument) */ \
  X(int, seq_age, 1)                      /*             a sequence's own step count minus pos_count (0 until it is loaded, copied in or reset: sl2_checkpoint.hip) */ \
  /* ---- stepping a subset of the batch (sl2_set_active_sequences) ---- */                                             \
  X(uint8_t, active, 1)                   /*             1 = the sequence takes part in the steps issued from now on (all ones after sl2_create); engine-global, in no blob */ \
  X(int, sel_gate, 1)                     /*             per step: n_sel of an active sequence, 0 of a paused one (k_select) - what the search kernels take for n_sel */ \
  X(int, m_gate, 1)                       /*             per step: m_count of an active sequence, 0 of a paused one (k_search_score) - what the update chain takes for m_count */ \
  /* ---- per-frame feature scratch, per slot ---- */                                                                              \
  X(double, f_h, N * 2)                   /* [N][2] */                                                                               \
  X(double, f_Hx, N * 14)                 /* [N][14] */                                                                              \
  X(double, f_Hy, N * 6)                  /* [N][6] */                                                                               \
  X(double, f_R, N)                       /* [N] */                                                                                  \
  X(double, f_S, N * 4)                   /* [N][4] */                                                                               \
  X(double, f_score, N)                   /* [N] */                                                                                  \
  X(double, f_z, N * 2)                   /* [N][2]      (persistent: untouched on failure, Q4) */                                   \
  X(double, f_nu, N * 2)                  /* [N][2] */                                                                               \
  X(int, sel_idx, N)                      /* [N]         selected feature slots in selection order */                                \
  X(int, n_sel, 1)                                                                                                                 \
  X(int, n_vis, 1)                                                                                                                 \
  X(int, meas_ok, N)                      /* [N]         per selected position k */                                                  \
  X(double, meas_score, N)                /* [N] */                                                                                  \
  X(int, succ_idx, N)                     /* [N]         successful feature slots, ascending (slot order) */                         \
  X(int, f_arow, N)                       /* [N]         per slot: first row of A^T / S of its measurement (2 x rank among the successes), -1 = none this frame */ \
  X(int, m_count, 1)                      /*             number of successful features (m = 2 * m_count) */                          \
  X(double, work, kWorkDoubles)           /* [kWorkDoubles]  window bytes, searched, candidates, exact-fallback searches, candidate tiles */ \
  X(int, srch_i, N * 8)                   /* [N][8]      per-feature search window: ucentre, vcentre, urelstart, nu, vrelstart, nv, hw, hh */ \
  X(double, srch_d, N * 4)                /* [N][4]      PuInv (a, b, c), pad */                                                     \
  X(int, srch_res, N * 8)                 /* [N][8]      per selected position: code, u, v, S1, S2, X, ncand, pad */                 \
  X(int, srch_sel, N * 16)                /* [N][16]     per selected position k (written by k_select): slot f, the 7 window ints of srch_i, then PuInv (a, b, c) as 3 doubles, pad - one 64-byte line, so that the search kernel needs ONE round trip for it */ \
  /* ---- EKF update workspaces ---- */                                                                                            \
  X(double, At, mld * ld)                 /* [mld][ld]   (P H^T)^T, k-major; column ld-1 carries nu */                               \
  X(double, Vt, mld * ld)                 /* [mld][ld]   L^-1 (P H^T)^T */                                                           \
  X(double, St, mld * mld)                /* [mld][mld]  St[c][r] = S[r][c]; overwritten by L (same layout) */                       \
  X(double, LinvT, nblk_max * 1024)       /* [nblk_max][32][32]  LinvT[p][k] = (L_JJ^-1)[k][p] */                                    \
  /* ---- feature initialisation ---- */                                                                      \
  X(int, part_i, kPartInts)               /* [kPartInts] */                                                                          \
  X(double, part_d, kPartDoubles)         /* [kPartDoubles]  [2] = evbest of the last detection */                                   \
  X(int, ps_i, kpart * kPsInts)           /* [kpart][kPsInts] */                                                                     \
  X(double, ps_d, kpart * kPsDoubles)     /* [kpart][kPsDoubles] */                                                                  \
  /* Q28 (feature.cpp:254): a conversion moves the LATER features' position_in_total_state_vector_ by 6 instead of 3, and the   */ \
  /* reference then places their dh_by_dy blocks three columns early in H (monoslam.cpp:564).  pos_err = how far a slot's       */ \
  /* recorded position lies below its true one; f_hcol = the engine column its H block therefore lands on (k_search_score       */ \
  /* recomputes it for sequences that carry such an error; every other sequence uses 13 + 3 slot).                              */ \
  X(int, pos_err, N)                      /* [N] */                                                                                  \
  X(int, pos_err_any, 1)                                                                                                           \
  X(int, f_hcol, N)                       /* [N] */                                                                                  \
  X(double, particles, kpart * pcap * kParticleDoubles)   /* [kpart][pcap][kParticleDoubles] */                                    \
  X(unsigned long long, rand48, 1)        /*             drand48 state (srand48(0) at Init, monoslam.cpp:1968) */                    \
  X(double, prev_r, 3)                    /* [3]         camera position before the prediction (speed estimate, :121-124) */         \
  X(int, me_desc, kpart * pcap * 8)       /* [kpart][pcap][8]  search ellipses of the particles */                                   \
  /* ---- engine state of a sequence that no sequence blob carries (sl2_common.hpp says who reads and writes each) ---- */         \
  X(int, step_mark, 1)                    /*             1 = took part in the last make_measurements (sl2_get_step_stats) */ \
  X(double, seq_time, kSeqTimeDoubles)    /* [kSeqTimeDoubles]  nominal time step, time owed, step last used, catch-up switch (sl2_set_delta_t) */ \
  X(double, seq_cam, kSeqCamDoubles)      /* [kSeqCamDoubles]   fku, fkv, u0, v0, kd1, sd, two spare words (sl2_set_cameras) */

// The pointers themselves: sl2_engine derives from this, so that e->x, g->f_hcol and the rest are plain members.
struct SeqArrays {
#define SL2_X(type, name, elems) type* name = nullptr;
  SL2_SEQ_ARRAYS(SL2_X)
#undef SL2_X
};

// The arrays as a group whose first sequence is `first` sees them: every pointer advanced by first * elements per sequence.
inline SeqArrays seq_arrays_view(const SeqArrays& root, const SeqDims& d, size_t first) {
  const size_t N = d.N, ld = d.ld, mld = d.mld, nblk_max = d.nblk_max, kpart = d.kpart, pcap = d.pcap;
  SeqArrays v;
#define SL2_X(type, name, elems) v.name = root.name + first * (size_t)(elems);
  SL2_SEQ_ARRAYS(SL2_X)
#undef SL2_X
  return v;
}

// Group k of G contiguous groups over B sequences: B / G each, the first B % G groups one longer.
inline void group_range(int B, int G, int k, int* first, int* count) {
  const int base = B / G, rem = B % G;
  *first = k * base + (k < rem ? k : rem);
  *count = base + (k < rem ? 1 : 0);
}

}  // namespace sl2
