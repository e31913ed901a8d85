// Three physically different cameras of one image size in ONE batch (C ABI): each sequence has its own calibration - focal
// lengths, principal point, distortion, measurement noise - given once with sl2_set_cameras; the engine was created for the
// image size with the first camera's.  All three move along the same path over the same textured plane; per engine step:
//
//   sl2_synth_render_host      each camera's frame, rendered with that camera's OWN calibration
//   sl2_go_one_step            one launch sequence for the whole batch
//
// The scene is synthetic and made here; each camera's dozen known features are cut from its own first view.  The last lines are
// each camera's calibration as sl2_get_cameras reports it and its position error against the pose its last frame was rendered
// from - and, with --wrong, what happens to cameras 1 and 2 when the batch is left on the first camera's calibration.
//
//   mixed_camera_monoslam [--steps K] [--wrong]
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
  bool wrong = false;
  for (int i = 1; i < argc; ++i) {
    const std::string a = argv[i];
    if (a == "--steps" && i + 1 < argc) steps = atoi(argv[++i]);
    else if (a == "--wrong") wrong = true;
    else { fprintf(stderr, "usage: %s [--steps K] [--wrong]\n", argv[0]); return 2; }
  }
  if (steps < 2) steps = 2;
  if (sl2_device_count() < 1) { fprintf(stderr, "no HIP device: this engine has no CPU path\n"); return 3; }
  const int B = 3;
  sl2_camera cams[B];
  memset(cams, 0, sizeof(cams));
  cams[0].width = 320; cams[0].height = 240; cams[0].fku = 195; cams[0].fkv = 195; cams[0].u0 = 162; cams[0].v0 = 125; cams[0].kd1 = 9e-06; cams[0].sd = 1;
  cams[1] = cams[0]; cams[1].fku *= 1.07; cams[1].fkv *= 0.94; cams[1].u0 += 9.5; cams[1].v0 -= 6.25; cams[1].kd1 *= 2;
  cams[2] = cams[0]; cams[2].fku *= 0.9; cams[2].kd1 = 0.0; cams[2].sd = 2;
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
  const size_t fb = (size_t)cams[0].width * cams[0].height;
  double pose0[7];
  pose_at(0.0, pose0);
  double xv[13], Pxx[169] = {0};
  memcpy(xv, pose0, sizeof(pose0));
  velocity_at(0.0, xv + 7);
  xv[10] = 0.0; xv[11] = 0.0; xv[12] = kRoll;
  Pxx[0] = Pxx[14] = Pxx[28] = 0.0004;

  sl2_engine* eng = nullptr;
  CHECK(sl2_create(&cams[0], &prm, B, 32, 0, nullptr, &eng));      // the image size of the batch; every sequence starts on cams[0]
  if (!wrong) CHECK(sl2_set_cameras(eng, 1, B - 1, &cams[1]));     // ... and the other two get their own
  const int n_known = 12;
  std::vector<uint8_t> frames(B * fb);
  for (int s = 0; s < B; ++s) {
    // a dozen known features on a 4 x 3 pixel grid of THIS camera's first view: the plane's point behind each pixel, its template
    const sl2_camera& cam = cams[s];
    uint8_t* frame0 = &frames[s * fb];
    CHECK(sl2_synth_render_host(&cam, tex.data(), kTex, kTexExtent, origin, pose0, 1, frame0));
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
    CHECK(sl2_set_vehicle_state(eng, s, 1, xv, Pxx));
    CHECK(sl2_add_known_features(eng, s, 1, n_known, y.data(), xp.data(), patches.data()));
  }
  printf("3 cameras, %d known features each, %d engine steps%s\n", n_known, steps, wrong ? "; all three left on camera 0's calibration" : "");

  double shown[7];
  memcpy(shown, pose0, sizeof(pose0));
  for (int k = 0; k < steps; ++k) {
    pose_at((k + 1) * prm.delta_t, shown);
    for (int s = 0; s < B; ++s)
      CHECK(sl2_synth_render_host(&cams[s], tex.data(), kTex, kTexExtent, origin, shown, 1, &frames[s * fb]));
    CHECK(sl2_go_one_step(eng, frames.data(), fb, /*frames_on_device=*/0, /*save_trajectory=*/0, /*enable_mapping=*/0));
    CHECK(sl2_synchronize(eng));                        // (host frames: the buffer is rendered into again next step)
  }
  sl2_camera got[B];
  CHECK(sl2_get_cameras(eng, 0, B, got));
  for (int s = 0; s < B; ++s) {
    double x13[13], P[169];
    int32_t counters[3], labels[32];
    CHECK(sl2_get_vehicle_state(eng, s, 1, x13, P));
    CHECK(sl2_get_selection(eng, s, labels, 32, counters));
    const double ex = x13[0] - shown[0], ey = x13[1] - shown[1], ez = x13[2] - shown[2];
    printf("camera %d  fku %.3f fkv %.3f u0 %.3f v0 %.3f kd1 %.3e sd %d  r = (% .4f % .4f % .4f)  position error %.6f m  visible %d  selected %d\n",
           s, got[s].fku, got[s].fkv, got[s].u0, got[s].v0, got[s].kd1, got[s].sd, x13[0], x13[1], x13[2],
           std::sqrt(ex * ex + ey * ey + ez * ez), counters[0], counters[1]);
  }
  sl2_destroy(eng);
  return 0;
}
