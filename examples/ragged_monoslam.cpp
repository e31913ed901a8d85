// Sequences of unequal length in ONE batch (C ABI): every directory is a camera that runs for as long as it has frames, and
// the batch is stepped until the longest one ends.  Per frame:
//
//   sl2_ingest_next_ragged     frame k of every sequence that still has one, have[s] = 1 for those
//   sl2_set_active_sequences   have[] is the mask: a sequence that has ended is left exactly as its last frame left it
//   sl2_go_one_step            one launch sequence for the whole batch, whatever the mask
//
//   ragged_monoslam --cfg scene.cfg --frames dir0 --frames dir1 [--frames dir2 ...] [--mapping]
//
// Every sequence starts from the state and the known features of scene.cfg (the keys of examples/headless_monoslam).  The
// last line per sequence is what examples/monoslam_adapter prints for its last frame when it is run on that directory alone.
#include "scene_cfg.hpp"

#define CHECK(call)                                                                        \
  do {                                                                                     \
    const int rc_ = (call);                                                                \
    if (rc_ != SL2_OK) { fprintf(stderr, "%s -> %d: %s\n", #call, rc_, sl2_last_error()); return 1; } \
  } while (0)

int main(int argc, char** argv) {
  std::string cfg;
  std::vector<std::string> frame_dirs;
  int mapping = 0;
  for (int i = 1; i < argc; ++i) {
    const std::string a = argv[i];
    if (a == "--cfg" && i + 1 < argc) cfg = argv[++i];
    else if (a == "--frames" && i + 1 < argc) frame_dirs.push_back(argv[++i]);
    else if (a == "--mapping") mapping = 1;
    else { fprintf(stderr, "usage: %s --cfg scene.cfg --frames dir0 [--frames dir1 ...] [--mapping]\n", argv[0]); return 2; }
  }
  if (cfg.empty() || frame_dirs.empty()) { fprintf(stderr, "need --cfg and at least one --frames\n"); return 2; }
  Scene sc;
  if (int rc = load_scene(cfg, sc)) return rc;
  if (sl2_device_count() < 1) { fprintf(stderr, "no HIP device: this engine has no CPU path\n"); return 3; }
  const int B = (int)frame_dirs.size(), max_features = 128;
  sl2_engine* eng = nullptr;
  CHECK(sl2_create(&sc.cam, &sc.prm, B, max_features, 0, nullptr, &eng));
  for (int s = 0; s < B; ++s) {
    CHECK(sl2_set_vehicle_state(eng, s, 1, sc.xv, sc.Pxx));
    for (int k = 0; k < sc.n_known; ++k)
      CHECK(sl2_add_known_features(eng, s, 1, 1, &sc.y[3 * k], &sc.xp[7 * k], &sc.patches[121 * k]));
  }
  std::vector<const char*> dirs;
  for (const std::string& d : frame_dirs) dirs.push_back(d.c_str());
  sl2_ingest* grab = nullptr;
  CHECK(sl2_ingest_open(dirs.data(), B, sc.cam.width, sc.cam.height, 0, 8, &grab));
  std::vector<int32_t> counts(B);
  sl2_ingest_frame_counts(grab, counts.data(), B);
  int longest = 0;
  for (int s = 0; s < B; ++s) longest = counts[s] > longest ? counts[s] : longest;
  printf("%d sequences, %d known features each, %d steps, mapping %s\n", B, sc.n_known, longest, mapping ? "on" : "off");

  std::vector<uint8_t> have(B);
  for (int k = 0; k < longest; ++k) {
    const uint8_t* d_frames = nullptr;
    size_t stride = 0;
    CHECK(sl2_ingest_next_ragged(grab, sl2_get_stream(eng), &d_frames, &stride, have.data()));
    CHECK(sl2_set_active_sequences(eng, 0, B, have.data(), /*on_device=*/0));      // consumed before the call returns; no synchronisation
    CHECK(sl2_go_one_step(eng, d_frames, stride, /*frames_on_device=*/1, /*save_trajectory=*/1, mapping));
  }
  for (int s = 0; s < B; ++s) {
    double x13[13], P[169], pd[9];
    int32_t counters[3], labels[128], pi[16];
    std::vector<sl2_feature_info> feats(max_features);
    int nfeat = 0, measured = 0;
    CHECK(sl2_get_vehicle_state(eng, s, 1, x13, P));
    CHECK(sl2_get_selection(eng, s, labels, 128, counters));
    CHECK(sl2_get_features(eng, s, feats.data(), max_features, 0, &nfeat));
    CHECK(sl2_get_partial_feature(eng, s, 0, pi, pd, nullptr, 0));
    for (int i = 0; i < nfeat; ++i) measured += (feats[i].selected_flag && feats[i].successful_measurement_flag) ? 1 : 0;
    printf("sequence %d  frame %4d  r = (% .4f % .4f % .4f)  features %d  visible %d  selected %d  measured %d  partial %d\n", s,
           counts[s] - 1, x13[0], x13[1], x13[2], nfeat, counters[0], counters[1], measured, pi[0]);
  }
  sl2_ingest_close(grab);
  sl2_destroy(eng);
  return 0;
}
