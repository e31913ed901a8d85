// Cameras that misbehave, and the gate that notices (C ABI): the frame monitor in front of the step.
//
// Three cameras move along the same path over the same textured plane, each in the batch twice:
//
//   camera 0   repeats its last buffer for five frames (a stalled driver)
//   camera 1   delivers three black frames (an exposure glitch)
//   camera 2   the control: every frame is good
//
// Sequences 0 .. 2 are fed through the gate chain, sequences 3 .. 5 are fed the same frames with every rule off.  Per engine step:
//
//   sl2_examine_frames          statistics, verdict and an active byte per sequence, two launches on the engine's stream
//   sl2_set_active_sequences    the active bytes, in device form: a rejected frame's sequence sits the step out
//   sl2_go_one_step             the whole batch
//
// with sl2_set_pause_catch_up on, so the predict that follows a gap covers it.  No host round trip lies between the three.  A
// repeated frame is the worst case for a constant-velocity filter - the image shows no motion, the update pulls the velocity to
// zero, and the next real frame is a jump -; the position errors at the end show what the gate is worth.
//
//   frame_gate_monoslam [--steps K]
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
  int steps = 24;
  for (int i = 1; i < argc; ++i) {
    const std::string a = argv[i];
    if (a == "--steps" && i + 1 < argc) steps = atoi(argv[++i]);
    else { fprintf(stderr, "usage: %s [--steps K]\n", argv[0]); return 2; }
  }
  if (steps < 16) steps = 16;
  if (sl2_device_count() < 1) { fprintf(stderr, "no HIP device: this engine has no CPU path\n"); return 3; }
  const int NC = 3, B = 6;          // cameras; sequences: every camera behind the gate and without it
  const int kFirstBad = 8, kRepeats = 5, kBlacks = 3;
  sl2_camera cam;
  memset(&cam, 0, sizeof(cam));
  cam.width = 320; cam.height = 240; cam.fku = 195; cam.fkv = 195; cam.u0 = 162; cam.v0 = 125; cam.kd1 = 9e-06; cam.sd = 1;
  const size_t fb = (size_t)cam.width * cam.height;
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
  sl2_frame_monitor* mon = nullptr;
  void *d_frames_v = nullptr, *d_active_v = nullptr, *d_verdict_v = nullptr;
  CHECK(sl2_create(&cam, &prm, B, 32, 0, nullptr, &eng));
  CHECK(sl2_frame_monitor_create(0, B, cam.width, cam.height, &mon));
  CHECK(sl2_dev_malloc(0, B * fb, &d_frames_v));
  CHECK(sl2_dev_malloc(0, B, &d_active_v));
  CHECK(sl2_dev_malloc(0, B * sizeof(uint32_t), &d_verdict_v));
  uint8_t* d_frames = (uint8_t*)d_frames_v;

  // the gate of sequences 0 .. 2: a repeated buffer, a frame with more than half its pixels in the darkest bin, a frame without
  // range.  Sequences 3 .. 5 keep the gate of a new monitor: every rule off, every frame passes.
  sl2_frame_gate gate;
  memset(&gate, 0, sizeof(gate));
  gate.reject_repeated = 1; gate.dark_bins = 1; gate.max_dark_pixels = (uint32_t)(fb / 2); gate.min_range = 16;
  const sl2_frame_gate gates[NC] = {gate, gate, gate};
  CHECK(sl2_frame_monitor_set_gates(mon, 0, NC, gates));
  CHECK(sl2_set_pause_catch_up(eng, 1));

  // a dozen known features on a 4 x 3 pixel grid of the first view: the plane's point behind each pixel, its template
  std::vector<uint8_t> good(fb), frames(B * fb);
  CHECK(sl2_synth_render_host(&cam, tex.data(), kTex, kTexExtent, origin, pose0, 1, good.data()));
  const int n_known = 12;
  std::vector<double> y(3 * n_known), xp(7 * n_known);
  std::vector<uint8_t> patches(121 * n_known);
  for (int k = 0; k < n_known; ++k) {
    const int u = 60 + (k % 4) * 66, v = 50 + (k / 4) * 70;
    const double c0 = u - cam.u0, c1 = v - cam.v0, factor = std::sqrt(1 - 2 * cam.kd1 * (c0 * c0 + c1 * c1));
    const double ray[3] = {(c0 / factor) / -cam.fku, (c1 / factor) / -cam.fkv, 1.0}, t = -pose0[2] / ray[2];
    y[3 * k] = pose0[0] + t * ray[0]; y[3 * k + 1] = pose0[1] + t * ray[1]; y[3 * k + 2] = 0.0;
    memcpy(&xp[7 * k], pose0, sizeof(pose0));
    for (int r = 0; r < 11; ++r) memcpy(&patches[121 * k + 11 * r], &good[(size_t)(v - 5 + r) * cam.width + u - 5], 11);
  }
  for (int b = 0; b < B; ++b) {
    CHECK(sl2_set_vehicle_state(eng, b, 1, xv, Pxx));
    CHECK(sl2_add_known_features(eng, b, 1, n_known, y.data(), xp.data(), patches.data()));
  }
  printf("3 cameras, each behind the gate and without it, %d known features each, %d engine steps; camera 0 repeats its buffer in steps "
         "%d .. %d, camera 1 is black in steps %d .. %d\n", n_known, steps, kFirstBad, kFirstBad + kRepeats - 1, kFirstBad, kFirstBad + kBlacks - 1);

  std::vector<uint8_t> last_of_camera0(fb);
  std::vector<uint32_t> verdict(B);
  int rejected[B] = {0, 0, 0, 0, 0, 0};
  double shown[7], worst[B] = {0, 0, 0, 0, 0, 0};
  memcpy(shown, pose0, sizeof(pose0));
  for (int k = 0; k < steps; ++k) {
    pose_at((k + 1) * prm.delta_t, shown);
    CHECK(sl2_synth_render_host(&cam, tex.data(), kTex, kTexExtent, origin, shown, 1, good.data()));
    const bool repeat = k >= kFirstBad && k < kFirstBad + kRepeats, black = k >= kFirstBad && k < kFirstBad + kBlacks;
    if (!repeat) last_of_camera0 = good;
    for (int half = 0; half < 2; ++half) {
      memcpy(&frames[(half * NC + 0) * fb], last_of_camera0.data(), fb);
      if (black) memset(&frames[(half * NC + 1) * fb], 0, fb); else memcpy(&frames[(half * NC + 1) * fb], good.data(), fb);
      memcpy(&frames[(half * NC + 2) * fb], good.data(), fb);
    }
    CHECK(sl2_dev_upload(0, d_frames, frames.data(), B * fb));
    CHECK(sl2_examine_frames(mon, sl2_get_stream(eng), d_frames, fb, nullptr, nullptr, (uint32_t*)d_verdict_v, (uint8_t*)d_active_v));
    CHECK(sl2_set_active_sequences(eng, 0, B, (const uint8_t*)d_active_v, /*on_device=*/1));
    CHECK(sl2_go_one_step(eng, d_frames, fb, /*frames_on_device=*/1, /*save_trajectory=*/0, /*enable_mapping=*/0));
    CHECK(sl2_synchronize(eng));                        // (the device frames are written again next step)
    CHECK(sl2_dev_download(0, verdict.data(), d_verdict_v, B * sizeof(uint32_t)));
    for (int b = 0; b < B; ++b) {
      double state[13], P[169];
      CHECK(sl2_get_vehicle_state(eng, b, 1, state, P));
      const double ex = state[0] - shown[0], ey = state[1] - shown[1], ez = state[2] - shown[2], e = std::sqrt(ex * ex + ey * ey + ez * ez);
      if (verdict[b] != 0) ++rejected[b];
      else if (e > worst[b]) worst[b] = e;              // the error while the camera's frames are good: the jump after a gap shows here
    }
    if (k >= kFirstBad - 1 && k <= kFirstBad + kRepeats)
      printf("step %2d  verdicts %2u %2u %2u | %u %u %u\n", k, verdict[0], verdict[1], verdict[2], verdict[3], verdict[4], verdict[5]);
  }

  static const char* kName[NC] = {"repeats its buffer", "black frames", "control"};
  for (int s = 0; s < NC; ++s) {
    double state[2][13], P[169], err[2];
    for (int half = 0; half < 2; ++half) {
      CHECK(sl2_get_vehicle_state(eng, half * NC + s, 1, state[half], P));
      const double ex = state[half][0] - shown[0], ey = state[half][1] - shown[1], ez = state[half][2] - shown[2];
      err[half] = std::sqrt(ex * ex + ey * ey + ez * ez);
    }
    printf("camera %d (%s)  rejected %d  position error with the gate %.6f m (worst on a good frame %.6f m)  without %.6f m (worst %.6f m)\n", s,
           kName[s], rejected[s], err[0], worst[s], err[1], worst[NC + s]);
  }
  sl2_frame_monitor_destroy(mon);
  sl2_dev_free(0, d_frames_v);
  sl2_dev_free(0, d_active_v);
  sl2_dev_free(0, d_verdict_v);
  sl2_destroy(eng);
  return 0;
}
