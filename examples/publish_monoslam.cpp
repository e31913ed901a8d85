// A publisher in front of a batch (C ABI): four cameras replay the recording of scene.cfg - three of them drop a frame now and
// then, so that their maps and trajectories differ - and after EVERY frame the pose and the map of every sequence are read out in
// one call,
//
//   sl2_snapshot_batch         three launches, one wait and one copy for all sequences: only the sections asked for
//                              (SL2_SNAP_POSE | SL2_SNAP_FEATURES | SL2_SNAP_SELECTION here), packed back to back
//
// and a digest line per sequence is printed: what a service would put on the wire.  With --single the same lines are built from
// one sl2_snapshot per sequence instead (B launches, B waits, the full blob each): the two outputs must be identical.
//
//   publish_monoslam --cfg scene.cfg --frames dir [--mapping] [--single]
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

static uint64_t fnv1a(uint64_t h, const void* data, size_t n) {
  const unsigned char* p = (const unsigned char*)data;
  for (size_t i = 0; i < n; ++i) h = (h ^ p[i]) * 1099511628211ull;
  return h;
}

// The line of one sequence from its blob, whichever call packed it: the counts, the camera position and a digest over xv_, Pxx_,
// the feature records and the selection (the sections both kinds of blob carry; a section is [its offset, the next offset)).
static void publish(int frame, const unsigned char* blob) {
  const sl2_snapshot_header* h = (const sl2_snapshot_header*)blob;
  const double* xv = (const double*)(blob + h->off_xv);
  uint64_t d = 14695981039346656037ull;
  d = fnv1a(d, blob + h->off_xv, (size_t)(h->off_features - h->off_xv));
  d = fnv1a(d, blob + h->off_features, (size_t)(h->off_cov - h->off_features));
  d = fnv1a(d, blob + h->off_selection, (size_t)(h->off_traj - h->off_selection));
  printf("frame %3d seq %d  own steps %3d  features %2d  selected %2d  partial %d  r %+.9f %+.9f %+.9f  digest %016llx\n", frame, h->seq,
         h->sequence_steps, h->n_features, h->n_selected, h->n_partial, xv[0], xv[1], xv[2], (unsigned long long)d);
}

int main(int argc, char** argv) {
  std::string cfg, frames_dir;
  bool mapping = false, single = false;
  for (int i = 1; i < argc; ++i) {
    const std::string a = argv[i];
    if (a == "--cfg" && i + 1 < argc) cfg = argv[++i];
    else if (a == "--frames" && i + 1 < argc) frames_dir = argv[++i];
    else if (a == "--mapping") mapping = true;
    else if (a == "--single") single = true;
    else { fprintf(stderr, "usage: %s --cfg scene.cfg --frames dir [--mapping] [--single]\n", argv[0]); return 2; }
  }
  if (cfg.empty() || frames_dir.empty()) { fprintf(stderr, "need --cfg and --frames\n"); return 2; }
  Scene sc;
  if (int rc = load_scene(cfg, sc)) return rc;
  std::vector<std::string> paths;
  if (list_dir(frames_dir, paths) || paths.empty()) { fprintf(stderr, "cannot list %s: %s\n", frames_dir.c_str(), sl2_last_error()); return 1; }
  if (sl2_device_count() < 1) { fprintf(stderr, "no HIP device: this engine has no CPU path\n"); return 3; }
  const int B = 4, max_features = 32;
  const size_t fb = (size_t)sc.cam.width * sc.cam.height;
  sl2_engine* eng = nullptr;
  CHECK(sl2_create(&sc.cam, &sc.prm, B, max_features, 0, nullptr, &eng));
  for (int s = 0; s < B; ++s) {
    CHECK(sl2_set_vehicle_state(eng, s, 1, sc.xv, sc.Pxx));
    for (int k = 0; k < sc.n_known; ++k) CHECK(sl2_add_known_features(eng, s, 1, 1, &sc.y[3 * k], &sc.xp[7 * k], &sc.patches[121 * k]));
  }
  const int sections = SL2_SNAP_POSE | SL2_SNAP_FEATURES | SL2_SNAP_SELECTION;
  // no blob of this engine restricted to these sections is larger: the shape as sl2_create derives it from the parameters
  const int kpart = sc.prm.max_features_to_init_at_once < 1 ? 1 : (sc.prm.max_features_to_init_at_once > 4 ? 4 : sc.prm.max_features_to_init_at_once);
  const int np = sc.prm.number_of_particles < 1 ? 1 : (sc.prm.number_of_particles > 1024 ? 1024 : sc.prm.number_of_particles);
  const size_t bound = sl2_snapshot_bound(max_features, kpart, (np + 63) / 64 * 64, sections);
  std::vector<unsigned char> packed(bound * B);
  std::vector<uint64_t> offsets(B + 1);
  printf("%d sequences, %d known features each, %d frames, %s; at most %zu bytes a frame (a full blob: up to %zu a sequence)\n", B, sc.n_known,
         (int)paths.size(), single ? "one sl2_snapshot per sequence" : "one sl2_snapshot_batch per frame", packed.size(), sl2_snapshot_capacity(eng));

  std::vector<uint8_t> frames(B * fb);
  std::vector<uint8_t> active(B);
  size_t published = 0;
  for (int k = 0; k < (int)paths.size(); ++k) {
    int w = 0, h = 0;
    if (sl2_read_image(paths[(size_t)k].c_str(), frames.data(), fb, &w, &h) != SL2_OK || w != sc.cam.width || h != sc.cam.height) {
      fprintf(stderr, "%s: %s\n", paths[(size_t)k].c_str(), sl2_last_error());
      return 1;
    }
    for (int s = 1; s < B; ++s) memcpy(&frames[s * fb], frames.data(), fb);
    for (int s = 0; s < B; ++s) active[s] = (s == 0 || (k + 1) % (s + 3) != 0) ? 1 : 0;      // camera s > 0 drops every (s + 3)rd frame
    CHECK(sl2_set_active_sequences(eng, 0, B, active.data(), /*mask_on_device=*/0));
    CHECK(sl2_go_one_step(eng, frames.data(), fb, /*frames_on_device=*/0, /*save_trajectory=*/1, /*enable_mapping=*/mapping ? 1 : 0));
    if (single) {
      for (int s = 0; s < B; ++s) {
        const void* blob = nullptr;
        size_t bytes = 0;
        CHECK(sl2_snapshot(eng, s, /*traj_cursor=*/0, /*patch_from_label=*/0, &blob, &bytes));
        publish(k, (const unsigned char*)blob);
        published += bytes;
      }
    } else {
      CHECK(sl2_snapshot_batch(eng, 0, B, sections, /*cursors=*/nullptr, packed.data(), packed.size(), offsets.data(), /*on_device=*/0));
      for (int s = 0; s < B; ++s) publish(k, &packed[offsets[(size_t)s]]);
      published += offsets[(size_t)B];
    }
  }
  fprintf(stderr, "%zu bytes crossed the bus for %d frames\n", published, (int)paths.size());
  sl2_destroy(eng);
  return 0;
}
