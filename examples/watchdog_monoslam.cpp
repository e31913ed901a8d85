// A watchdog over a batch (C ABI): four cameras replay the recording of scene.cfg; from frame F on, one of them is handed the
// frames of ANOTHER recording - a feed that was mixed up - and its filter loses the map.  The loop reads the whole batch's
// consistency record after every step,
//
//   sl2_get_step_stats         one launch, one synchronisation for all sequences: matched features, NIS with its degrees of
//                              freedom, log det S, the worst feature
//
// and when a sequence has matched nothing for K steps in a row it is reset (sl2_reset_sequences), given the scene's initial
// state and known features again, and its own recording is replayed from the start; the other sequences never notice.
//
//   watchdog_monoslam --cfg scene.cfg --frames dir --wrong other_dir [--victim 2] [--from 8] [--patience 3]
//
// NIS bounds (chi-square with `dof` degrees of freedom) are the caller's business - a table or a statistics library; this
// example only prints the figure next to the count it acts on.
#include "scene_cfg.hpp"

#define CHECK(call)                                                                        \
  do {                                                                                     \
    const int rc_ = (call);                                                                \
    if (rc_ != SL2_OK) { fprintf(stderr, "%s -> %d: %s\n", #call, rc_, sl2_last_error()); return 1; } \
  } while (0)

static int list_dir(const std::string& dir, std::vector<std::string>& paths) {
  int count = 0;
  if (sl2_list_frames(dir.c_str(), nullptr, 0, &count) != SL2_OK) return 1;
  std::vector<char> buf((size_t)count * 4096 + 1);
  if (sl2_list_frames(dir.c_str(), buf.data(), buf.size(), &count) != SL2_OK) return 1;
  const char* p = buf.data();
  for (int i = 0; i < count; ++i) {
    const char* e = strchr(p, '\n');
    paths.push_back(e ? std::string(p, e) : std::string(p));
    if (!e) break;
    p = e + 1;
  }
  return 0;
}

static int start_sequence(sl2_engine* eng, const Scene& sc, int s) {
  CHECK(sl2_set_vehicle_state(eng, s, 1, sc.xv, sc.Pxx));
  for (int k = 0; k < sc.n_known; ++k)
    CHECK(sl2_add_known_features(eng, s, 1, 1, &sc.y[3 * k], &sc.xp[7 * k], &sc.patches[121 * k]));
  return 0;
}

int main(int argc, char** argv) {
  std::string cfg, frames_dir, wrong_dir;
  int victim = 2, from = 8, patience = 3;
  for (int i = 1; i < argc; ++i) {
    const std::string a = argv[i];
    if (a == "--cfg" && i + 1 < argc) cfg = argv[++i];
    else if (a == "--frames" && i + 1 < argc) frames_dir = argv[++i];
    else if (a == "--wrong" && i + 1 < argc) wrong_dir = argv[++i];
    else if (a == "--victim" && i + 1 < argc) victim = atoi(argv[++i]);
    else if (a == "--from" && i + 1 < argc) from = atoi(argv[++i]);
    else if (a == "--patience" && i + 1 < argc) patience = atoi(argv[++i]);
    else { fprintf(stderr, "usage: %s --cfg scene.cfg --frames dir --wrong other_dir [--victim s] [--from F] [--patience K]\n", argv[0]); return 2; }
  }
  const int B = 4, max_features = 32;
  if (cfg.empty() || frames_dir.empty() || wrong_dir.empty() || victim < 0 || victim >= B || from < 0 || patience < 1) {
    fprintf(stderr, "need --cfg, --frames and --wrong; 0 <= victim < %d\n", B);
    return 2;
  }
  Scene sc;
  if (int rc = load_scene(cfg, sc)) return rc;
  std::vector<std::string> good, wrong;
  if (list_dir(frames_dir, good) || list_dir(wrong_dir, wrong) || good.empty() || wrong.empty()) {
    fprintf(stderr, "cannot list the frame directories: %s\n", sl2_last_error());
    return 1;
  }
  if (sl2_device_count() < 1) { fprintf(stderr, "no HIP device: this engine has no CPU path\n"); return 3; }
  const size_t fb = (size_t)sc.cam.width * sc.cam.height;
  auto read_frame = [&](const std::string& path, uint8_t* out) {
    int w = 0, h = 0;
    if (sl2_read_image(path.c_str(), out, fb, &w, &h) != SL2_OK || w != sc.cam.width || h != sc.cam.height) {
      fprintf(stderr, "%s: %s\n", path.c_str(), sl2_last_error());
      return 1;
    }
    return 0;
  };
  sl2_engine* eng = nullptr;
  CHECK(sl2_create(&sc.cam, &sc.prm, B, max_features, 0, nullptr, &eng));
  for (int s = 0; s < B; ++s)
    if (start_sequence(eng, sc, s)) return 1;
  const int steps = (int)good.size();
  printf("%d sequences, %d known features each, %d steps; sequence %d gets the wrong frames from step %d, patience %d\n", B, sc.n_known,
         steps, victim, from, patience);

  std::vector<uint8_t> frames(B * fb);
  std::vector<sl2_step_stats> rec(B);
  std::vector<int> cursor(B, 0), unmatched(B, 0);     // each sequence's place in its recording; steps in a row without a match
  bool feed_is_wrong = false;
  std::vector<int> resets(B, 0);
  for (int k = 0; k < steps; ++k) {
    if (k == from) feed_is_wrong = true;
    for (int s = 0; s < B; ++s) {
      const bool swapped = s == victim && feed_is_wrong;
      const std::string& path = swapped ? wrong[(size_t)k % wrong.size()] : good[(size_t)cursor[s] % good.size()];
      if (read_frame(path, &frames[s * fb])) return 1;
      cursor[s] += 1;
    }
    CHECK(sl2_go_one_step(eng, frames.data(), fb, /*frames_on_device=*/0, /*save_trajectory=*/0, /*enable_mapping=*/0));
    CHECK(sl2_get_step_stats(eng, 0, B, rec.data(), /*out_on_device=*/0));      // the whole batch; waits for the step
    for (int s = 0; s < B; ++s) {
      const sl2_step_stats& r = rec[s];
      unmatched[s] = (r.stepped && r.n_matched == 0) ? unmatched[s] + 1 : 0;
      printf("step %3d seq %d  own step %3d  matched %2d / %2d  dof %2d  nis %9.4f  log det S %9.3f  worst label %2d (d2 %.3f)%s\n", k, s,
             r.sequence_steps, r.n_matched, r.n_selected, r.dof, r.nis, r.log_det_S, r.worst_label, r.worst_feature_d2,
             r.status_flags ? "  STATUS" : "");
      if (unmatched[s] >= patience) {               // lost: start it again from the scene, on its own recording
        CHECK(sl2_reset_sequences(eng, s, 1));
        if (start_sequence(eng, sc, s)) return 1;
        cursor[s] = 0;
        unmatched[s] = 0;
        if (s == victim) feed_is_wrong = false;     // (the mixed-up feed has been put right)
        resets[s] += 1;
        printf("step %3d seq %d  RESET after %d steps without a match\n", k, s, patience);
      }
    }
  }
  CHECK(sl2_get_step_stats(eng, 0, B, rec.data(), 0));
  for (int s = 0; s < B; ++s)
    printf("final seq %d  own steps %d  matched %d  dof %d  resets %d\n", s, rec[s].sequence_steps, rec[s].n_matched, rec[s].dof, resets[s]);
  sl2_destroy(eng);
  return 0;
}
