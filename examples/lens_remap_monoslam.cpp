// A camera whose lens the filter's model does not describe, in front of a 320 x 240 engine (C ABI): the lens remap.  The camera
// delivers 640 x 480 GRAY8 frames under a strongly distorting lens (the renderer draws them: the reference's radial model with a
// large coefficient, SL2_LENS_RADIAL1), and sits in the batch twice, naming the same bytes of the raw buffer:
//
//   sequence 0   remapped into a PINHOLE target      sl2_lens_pinhole_camera: kd1 = 0, the lens's image plane at 320 x 240
//   sequence 1   remapped into a mild-kd1 target     the same focal lengths and centre, kd1 = 3e-6: less stretching at the edges
//   sequence 2   a control: the view rendered directly under the pinhole target at 320 x 240, past the converter
//   sequence 3   a control: the view rendered directly under the mild-kd1 target
//
// All move along the same path over the same textured plane.  Setup builds the two maps on the host (sl2_lens_map_host), fills
// two map slots (sl2_converter_set_map) and names each sequence's slot (sl2_converter_set_remaps); then per engine step:
//
//   sl2_convert_frames         two sequences -> two 320 x 240 grey frames through their maps: one launch (k_convert_remap)
//   sl2_go_one_step            the whole batch, on the converted device frames, every sequence under ITS target's calibration
//
// - what a caller of OpenCV does per frame on the host with cv::remap.  Every sequence's known features carry templates cut from
// ITS OWN first 320 x 240 frame.  The position errors are printed side by side; no claim is made about them here.
//
//   lens_remap_monoslam [--steps K]
#include <scenelib2_amd.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#define CHECK(call)                                                                        \
  do {                                                                                     \
    const int rc_ = (call);                                                                \
    if (rc_ != SL2_OK) { fprintf(stderr, "%s -> %d: %s\n", #call, rc_, sl2_last_error()); return 1; } \
  } while (0)

static const double kPi = 3.14159265358979323846;
static const int kTex = 1024;
static const double kTexExtent = 2.0, kDepth = 0.6;

// band-limited noise: uniform bytes, a 5 x 5 box sum twice (torus), mapped to mean 128 / sigma 40
static std::vector<uint8_t> make_texture() {
  std::vector<double> a((size_t)kTex * kTex), b(a.size());
  unsigned long long s = 0x9E3779B97F4A7C15ull;
  for (double& v : a) { s = s * 6364136223846793005ull + 1442695040888963407ull; v = (double)(s >> 56); }
  for (int pass = 0; pass < 2; ++pass) {
    for (int r = 0; r < kTex; ++r)
      for (int c = 0; c < kTex; ++c) { double t = 0; for (int d = -2; d <= 2; ++d) t += a[(size_t)r * kTex + ((c + d + kTex) % kTex)]; b[(size_t)r * kTex + c] = t; }
    for (int r = 0; r < kTex; ++r)
      for (int c = 0; c < kTex; ++c) { double t = 0; for (int d = -2; d <= 2; ++d) t += b[(size_t)((r + d + kTex) % kTex) * kTex + c]; a[(size_t)r * kTex + c] = t; }
  }
  double mean = 0, var = 0;
  for (double v : a) mean += v;
  mean /= (double)a.size();
  for (double v : a) var += (v - mean) * (v - mean);
  const double sd = std::sqrt(var / (double)a.size());
  std::vector<uint8_t> tex(a.size());
  for (size_t i = 0; i < a.size(); ++i) {
    const double v = std::floor((a[i] - mean) * (40.0 / sd) + 128.0 + 0.5);
    tex[i] = (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
  }
  return tex;
}

// the cameras' common path: velocity = a sinusoid per axis, a slow roll about the optical axis
static const double kAmp[3] = {0.05, 0.04, 0.02}, kFreq[3] = {0.3, 0.4, 0.25}, kPhase[3] = {0.5, 1.0, 2.0}, kRoll = 0.01;
static void velocity_at(double t, double v[3]) {
  for (int i = 0; i < 3; ++i) v[i] = kAmp[i] * std::sin(2 * kPi * kFreq[i] * t + kPhase[i]);
}
static void pose_at(double t, double pose[7]) {
  for (int i = 0; i < 3; ++i) {
    const double w = 2 * kPi * kFreq[i];
    pose[i] = kAmp[i] / w * (std::cos(kPhase[i]) - std::cos(w * t + kPhase[i]));
  }
  pose[2] -= kDepth;
  pose[3] = std::cos(kRoll * t / 2.0); pose[4] = 0.0; pose[5] = 0.0; pose[6] = std::sin(kRoll * t / 2.0);
}

int main(int argc, char** argv) {
  int steps = 20;
  for (int i = 1; i < argc; ++i) {
    const std::string a = argv[i];
    if (a == "--steps" && i + 1 < argc) steps = atoi(argv[++i]);
    else { fprintf(stderr, "usage: %s [--steps K]\n", argv[0]); return 2; }
  }
  if (steps < 2) steps = 2;
  if (sl2_device_count() < 1) { fprintf(stderr, "no HIP device: this engine has no CPU path\n"); return 3; }
  const int NS = 2, B = 4;      // sequences behind the converter; engine sequences (two controls)
  // the camera: 640 x 480 GRAY8, a row pitch with padding; its lens in the renderer's terms and as a sl2_lens
  sl2_frame_source cam_src;
  memset(&cam_src, 0, sizeof(cam_src));
  cam_src.width = 640; cam_src.height = 480; cam_src.format = SL2_PIX_GRAY8; cam_src.pitch = 656; cam_src.offset = 0;
  const size_t raw_bytes = (size_t)cam_src.pitch * cam_src.height, grey_max = (size_t)cam_src.width * cam_src.height;
  sl2_camera src_cam;
  memset(&src_cam, 0, sizeof(src_cam));
  src_cam.width = 640; src_cam.height = 480; src_cam.fku = 390; src_cam.fkv = 390; src_cam.u0 = 324; src_cam.v0 = 250; src_cam.kd1 = 2e-06; src_cam.sd = 1;
  sl2_lens lens;
  memset(&lens, 0, sizeof(lens));
  lens.model = SL2_LENS_RADIAL1; lens.width = src_cam.width; lens.height = src_cam.height;
  lens.fx = src_cam.fku; lens.fy = src_cam.fkv; lens.cx = src_cam.u0; lens.cy = src_cam.v0; lens.k[0] = src_cam.kd1;
  // the two targets: the calibrations the engine runs with
  sl2_camera target[2];
  CHECK(sl2_lens_pinhole_camera(&lens, 320, 240, /*sd=*/1, &target[0]));
  target[1] = target[0];
  target[1].kd1 = 3e-06;
  const sl2_camera& eng_cam = target[0];
  const size_t fb = (size_t)eng_cam.width * eng_cam.height;
  static const char* kMapName[3] = {"PINHOLE", "RADIAL", "NONE"};
  const int target_of[B] = {0, 1, 0, 1};
  sl2_frame_source src[NS] = {cam_src, cam_src};
  std::vector<int32_t> map[2];
  for (int m = 0; m < 2; ++m) {
    map[m].resize(2 * fb);
    CHECK(sl2_lens_map_host(&lens, &target[m], map[m].data()));
  }
  long border[2] = {0, 0};
  for (int m = 0; m < 2; ++m)
    for (size_t i = 0; i < fb; ++i) border[m] += map[m][2 * i] == SL2_REMAP_BORDER;

  sl2_params prm;
  memset(&prm, 0, sizeof(prm));
  prm.delta_t = 1.0 / 30.0;
  prm.number_of_features_to_select = 10; prm.number_of_features_to_keep_visible = 12; prm.max_features_to_init_at_once = 1;
  prm.min_lambda = 0.5; prm.max_lambda = 5.0; prm.number_of_particles = 100; prm.standard_deviation_depth_ratio = 0.3;
  prm.min_number_of_particles = 20; prm.prune_probability_threshold = 0.05;
  prm.erase_partially_init_feature_after_this_many_attempts = 10;
  prm.minimum_attempted_measurements_of_feature = 10; prm.successful_match_fraction = 0.5;

  const std::vector<uint8_t> tex = make_texture();
  const double origin[2] = {0.0, 0.0};
  double pose0[7];
  pose_at(0.0, pose0);
  double xv[13], Pxx[169] = {0};
  memcpy(xv, pose0, sizeof(pose0));
  velocity_at(0.0, xv + 7);
  xv[10] = 0.0; xv[11] = 0.0; xv[12] = kRoll;
  Pxx[0] = Pxx[14] = Pxx[28] = 0.0004;

  sl2_engine* eng = nullptr;
  sl2_converter* conv = nullptr;
  void *d_frames_v = nullptr, *d_tex = nullptr, *d_origin = nullptr, *d_pose = nullptr, *d_grey = nullptr;
  CHECK(sl2_create(&eng_cam, &prm, B, 32, 0, nullptr, &eng));
  for (int b = 0; b < B; ++b) CHECK(sl2_set_cameras(eng, b, 1, &target[target_of[b]]));
  CHECK(sl2_converter_create(0, NS, eng_cam.width, eng_cam.height, &conv));
  CHECK(sl2_converter_set_sources(conv, 0, NS, src));
  const int32_t slot_of[NS] = {0, 1};
  for (int m = 0; m < 2; ++m) CHECK(sl2_converter_set_map(conv, m, lens.width, lens.height, map[m].data()));
  CHECK(sl2_converter_set_remaps(conv, 0, NS, slot_of));
  CHECK(sl2_dev_malloc(0, B * fb, &d_frames_v));
  CHECK(sl2_dev_malloc(0, tex.size(), &d_tex));
  CHECK(sl2_dev_malloc(0, sizeof(origin), &d_origin));
  CHECK(sl2_dev_malloc(0, sizeof(pose0), &d_pose));
  CHECK(sl2_dev_malloc(0, grey_max, &d_grey));
  CHECK(sl2_dev_upload(0, d_tex, tex.data(), tex.size()));
  CHECK(sl2_dev_upload(0, d_origin, origin, sizeof(origin)));
  uint8_t* d_frames = (uint8_t*)d_frames_v;

  std::vector<uint8_t> raw(raw_bytes, 0), grey(grey_max), frames(B * fb);
  // what the camera sees of a pose: its view rendered on the device at its own size under its own lens, brought back and laid
  // out with its row pitch; the controls' frames rendered directly under the two targets
  auto render = [&](const double pose[7]) -> int {
    CHECK(sl2_dev_upload(0, d_pose, pose, 7 * sizeof(double)));
    CHECK(sl2_synth_render_device(0, nullptr, &src_cam, (const uint8_t*)d_tex, kTex, kTexExtent, (const double*)d_origin, (const double*)d_pose, 1,
                                  (uint8_t*)d_grey));
    CHECK(sl2_dev_download(0, grey.data(), d_grey, grey_max));
    for (int y = 0; y < cam_src.height; ++y) memcpy(&raw[(size_t)y * cam_src.pitch], &grey[(size_t)y * cam_src.width], cam_src.width);
    for (int b = NS; b < B; ++b)
      CHECK(sl2_synth_render_host(&target[target_of[b]], tex.data(), kTex, kTexExtent, origin, pose, 1, &frames[b * fb]));
    return 0;
  };

  const int n_known = 12;
  if (render(pose0)) return 1;
  for (int s = 0; s < NS; ++s)
    CHECK(sl2_remap_frame_host(&src[s], map[slot_of[s]].data(), raw.data(), raw_bytes, eng_cam.width, eng_cam.height, &frames[s * fb]));
  for (int b = 0; b < B; ++b) {
    // a dozen known features on a 4 x 3 pixel grid of THIS sequence's first 320 x 240 view: the plane's point behind each pixel,
    // its template cut from the sequence's own converted frame
    const sl2_camera& cam = target[target_of[b]];
    const uint8_t* frame0 = &frames[b * fb];
    std::vector<double> y(3 * n_known), xp(7 * n_known);
    std::vector<uint8_t> patches(121 * n_known);
    for (int k = 0; k < n_known; ++k) {
      const int u = 60 + (k % 4) * 66, v = 50 + (k / 4) * 70;
      const double c0 = u - cam.u0, c1 = v - cam.v0, factor = std::sqrt(1 - 2 * cam.kd1 * (c0 * c0 + c1 * c1));
      const double ray[3] = {(c0 / factor) / -cam.fku, (c1 / factor) / -cam.fkv, 1.0}, t = -pose0[2] / ray[2];
      y[3 * k] = pose0[0] + t * ray[0]; y[3 * k + 1] = pose0[1] + t * ray[1]; y[3 * k + 2] = 0.0;
      memcpy(&xp[7 * k], pose0, sizeof(pose0));
      for (int r = 0; r < 11; ++r) memcpy(&patches[121 * k + 11 * r], &frame0[(size_t)(v - 5 + r) * cam.width + u - 5], 11);
    }
    CHECK(sl2_set_vehicle_state(eng, b, 1, xv, Pxx));
    CHECK(sl2_add_known_features(eng, b, 1, n_known, y.data(), xp.data(), patches.data()));
  }
  printf("1 camera remapped into 2 targets, 2 controls, %d known features each, %d engine steps, %zu raw bytes a frame, border entries %ld and %ld of %zu\n",
         n_known, steps, raw_bytes, border[0], border[1], fb);
  printf("lens RADIAL1 %dx%d fx %.6f fy %.6f cx %.6f cy %.6f k0 %.6e\n", lens.width, lens.height, lens.fx, lens.fy, lens.cx, lens.cy, lens.k[0]);

  double shown[7];
  memcpy(shown, pose0, sizeof(pose0));
  for (int k = 0; k < steps; ++k) {
    pose_at((k + 1) * prm.delta_t, shown);
    if (render(shown)) return 1;
    CHECK(sl2_dev_upload(0, d_frames + NS * fb, &frames[NS * fb], (B - NS) * fb));      // the controls' frames, as they are
    CHECK(sl2_convert_frames(conv, sl2_get_stream(eng), raw.data(), raw_bytes, /*raw_on_device=*/0, d_frames, fb));
    CHECK(sl2_go_one_step(eng, d_frames, fb, /*frames_on_device=*/1, /*save_trajectory=*/0, /*enable_mapping=*/0));
    CHECK(sl2_synchronize(eng));                        // (the raw buffer and the device frames are written again next step)
  }

  int32_t flags[B], got_slot[NS];
  sl2_frame_source got[NS];
  CHECK(sl2_get_status_flags(eng, 0, B, flags));
  CHECK(sl2_converter_get_sources(conv, 0, NS, got));
  CHECK(sl2_converter_get_remaps(conv, 0, NS, got_slot));
  for (int b = 0; b < B; ++b) {
    double state[13], P[169];
    int32_t labels[32], counters[3];
    sl2_camera cam;
    CHECK(sl2_get_vehicle_state(eng, b, 1, state, P));
    CHECK(sl2_get_selection(eng, b, labels, 32, counters));
    CHECK(sl2_get_cameras(eng, b, 1, &cam));
    const double ex = state[0] - shown[0], ey = state[1] - shown[1], ez = state[2] - shown[2];
    const double err = std::sqrt(ex * ex + ey * ey + ez * ez);
    if (b < NS)
      printf("sequence %d  source %dx%d %s  map %s  ", b, got[b].width, got[b].height, "GRAY8", kMapName[got_slot[b]]);
    else
      printf("sequence %d  source %dx%d %s  map %s  ", b, cam.width, cam.height, "GRAY8", kMapName[2]);
    printf("fku %.6f fkv %.6f u0 %.6f v0 %.6f kd1 %.6e sd %d  position error %.6f m  visible %d  selected %d  measured %d  flags %d\n", cam.fku, cam.fkv,
           cam.u0, cam.v0, cam.kd1, cam.sd, err, counters[0], counters[1], counters[2], flags[b]);
  }
  sl2_converter_destroy(conv);
  sl2_dev_free(0, d_grey); sl2_dev_free(0, d_pose); sl2_dev_free(0, d_origin); sl2_dev_free(0, d_tex);
  sl2_dev_free(0, d_frames);
  sl2_destroy(eng);
  return 0;
}
