// Machine-vision cameras in front of a 320 x 240 engine (C ABI): global-shutter cameras deliver a raw Bayer mosaic or deep grey
// in 16-bit words, and the converter takes both as they come.
//
//   sequence 0   640 x 480    SL2_PIX_BAYER_RGGB8   SL2_RESIZE_LINEAR   a reduction by 2
//   sequence 1   1280 x 960   SL2_PIX_BAYER_GRBG8   SL2_RESIZE_AREA     a reduction by 4
//   sequence 2   1280 x 960   SL2_PIX_GRAY12        SL2_RESIZE_AREA     16-bit little-endian words, twelve bits significant
//   sequence 3   a control: the same view rendered directly at 320 x 240, past the converter
//
// All move along the same path over the same textured plane.  Each camera's frame is rendered on the device at ITS resolution
// under ITS calibration - the one whose sl2_scale_camera image is the engine's camera - and packed into its raw format on the
// host.  The scene is grey, so the mosaic carries the rendered grey at every site, and the GRAY12 words carry it shifted left by
// four with random low bits.  Then per engine step:
//
//   sl2_convert_frames         three sequences -> three 320 x 240 grey frames: one launch for the LINEAR one, one for the AREA two
//   sl2_go_one_step            the whole batch, on the converted device frames
//
// Every sequence's known features carry templates cut from ITS OWN converted first frame.
//
//   machine_vision_monoslam [--steps K]
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

// a grey image into the camera's raw format: a grey scene leaves its grey at every site of a mosaic, whatever the pattern; deep
// grey carries it in the top eight of its twelve bits, noise below
static void pack_raw(const sl2_frame_source& src, const uint8_t* grey, uint8_t* raw) {
  static unsigned long long noise = 0x2545F4914F6CDD1Dull;
  for (int y = 0; y < src.height; ++y) {
    uint8_t* row = raw + src.offset + (size_t)y * src.pitch;
    const uint8_t* g = grey + (size_t)y * src.width;
    for (int x = 0; x < src.width; ++x) {
      if (src.format == SL2_PIX_GRAY12) {
        noise = noise * 6364136223846793005ull + 1442695040888963407ull;
        const unsigned v = ((unsigned)g[x] << 4) | (unsigned)(noise >> 60);
        row[2 * x] = (uint8_t)(v & 255u); row[2 * x + 1] = (uint8_t)(v >> 8);
      } else {
        row[x] = g[x];
      }
    }
  }
}

static const char* format_name(int format) {
  switch (format) {
    case SL2_PIX_GRAY8: return "GRAY8";
    case SL2_PIX_GRAY12: return "GRAY12";
    case SL2_PIX_BAYER_RGGB8: return "BAYER_RGGB8";
    case SL2_PIX_BAYER_GRBG8: return "BAYER_GRBG8";
    default: return "?";
  }
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
  const int NC = 3, NS = 3, B = 4;      // cameras; sequences behind the converter (one per camera); engine sequences (one control)
  sl2_camera eng_cam;
  memset(&eng_cam, 0, sizeof(eng_cam));
  eng_cam.width = 320; eng_cam.height = 240; eng_cam.fku = 195; eng_cam.fkv = 195; eng_cam.u0 = 162; eng_cam.v0 = 125; eng_cam.kd1 = 9e-06; eng_cam.sd = 1;
  const size_t fb = (size_t)eng_cam.width * eng_cam.height;

  static const char* kFilterName[2] = {"LINEAR", "AREA"};
  sl2_frame_source cam_src[NC];
  memset(cam_src, 0, sizeof(cam_src));
  cam_src[0].width = 640; cam_src[0].height = 480; cam_src[0].format = SL2_PIX_BAYER_RGGB8; cam_src[0].pitch = 640;
  cam_src[1].width = 1280; cam_src[1].height = 960; cam_src[1].format = SL2_PIX_BAYER_GRBG8; cam_src[1].pitch = 1280;
  cam_src[2].width = 1280; cam_src[2].height = 960; cam_src[2].format = SL2_PIX_GRAY12; cam_src[2].pitch = 1280 * 2;
  size_t raw_bytes = 0, grey_max = 0;
  for (int c = 0; c < NC; ++c) {
    cam_src[c].offset = raw_bytes;
    raw_bytes += (size_t)cam_src[c].pitch * cam_src[c].height;
    const size_t g = (size_t)cam_src[c].width * cam_src[c].height;
    if (g > grey_max) grey_max = g;
  }
  sl2_camera src_cam[NC], scaled[NC];
  for (int c = 0; c < NC; ++c) {
    const double k = (double)cam_src[c].width / eng_cam.width;      // the source camera whose resized image is the engine's camera
    src_cam[c] = eng_cam;
    src_cam[c].width = cam_src[c].width; src_cam[c].height = cam_src[c].height;
    src_cam[c].fku = eng_cam.fku * k; src_cam[c].fkv = eng_cam.fkv * k;
    src_cam[c].u0 = (eng_cam.u0 + 0.5) * k - 0.5; src_cam[c].v0 = (eng_cam.v0 + 0.5) * k - 0.5;
    src_cam[c].kd1 = eng_cam.kd1 / (k * k);
    CHECK(sl2_scale_camera(&src_cam[c], eng_cam.width, eng_cam.height, &scaled[c]));
  }
  // the three sequences behind the converter: a camera each, the filter that suits its reduction
  const int cam_of[NS] = {0, 1, 2};
  const int32_t filter_of[NS] = {SL2_RESIZE_LINEAR, SL2_RESIZE_AREA, SL2_RESIZE_AREA};
  sl2_frame_source src[NS];
  for (int s = 0; s < NS; ++s) src[s] = cam_src[cam_of[s]];

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
  for (int b = 0; b < NS; ++b) CHECK(sl2_set_cameras(eng, b, 1, &scaled[cam_of[b]]));      // (the control keeps the engine's camera)
  CHECK(sl2_converter_create(0, NS, eng_cam.width, eng_cam.height, &conv));
  CHECK(sl2_converter_set_filters(conv, 0, NS, filter_of));
  CHECK(sl2_converter_set_sources(conv, 0, NS, src));
  CHECK(sl2_dev_malloc(0, B * fb, &d_frames_v));
  CHECK(sl2_dev_malloc(0, tex.size(), &d_tex));
  CHECK(sl2_dev_malloc(0, sizeof(origin), &d_origin));
  CHECK(sl2_dev_malloc(0, sizeof(pose0), &d_pose));
  CHECK(sl2_dev_malloc(0, grey_max, &d_grey));
  CHECK(sl2_dev_upload(0, d_tex, tex.data(), tex.size()));
  CHECK(sl2_dev_upload(0, d_origin, origin, sizeof(origin)));
  uint8_t* d_frames = (uint8_t*)d_frames_v;

  std::vector<uint8_t> raw(raw_bytes, 0), grey(grey_max), frames(B * fb);
  // what the cameras see of a pose: each one's view rendered on the device at its own size, brought back and packed into its raw
  // format; the control's frame rendered directly at the engine's size
  auto render = [&](const double pose[7]) -> int {
    CHECK(sl2_dev_upload(0, d_pose, pose, 7 * sizeof(double)));
    for (int c = 0; c < NC; ++c) {
      const size_t g = (size_t)cam_src[c].width * cam_src[c].height;
      CHECK(sl2_synth_render_device(0, nullptr, &src_cam[c], (const uint8_t*)d_tex, kTex, kTexExtent, (const double*)d_origin, (const double*)d_pose, 1,
                                    (uint8_t*)d_grey));
      CHECK(sl2_dev_download(0, grey.data(), d_grey, g));
      pack_raw(cam_src[c], grey.data(), raw.data());
    }
    CHECK(sl2_synth_render_host(&eng_cam, tex.data(), kTex, kTexExtent, origin, pose, 1, &frames[NS * fb]));
    return 0;
  };

  const int n_known = 12;
  if (render(pose0)) return 1;
  for (int s = 0; s < NS; ++s)
    CHECK(sl2_convert_frame_host_filtered(&src[s], filter_of[s], raw.data(), raw_bytes, eng_cam.width, eng_cam.height, &frames[s * fb]));
  for (int b = 0; b < B; ++b) {
    // a dozen known features on a 4 x 3 pixel grid of THIS sequence's first 320 x 240 view: the plane's point behind each pixel,
    // its template cut from the sequence's own converted frame
    const sl2_camera& cam = b < NS ? scaled[cam_of[b]] : eng_cam;
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
  printf("3 machine-vision cameras, 1 control, %d known features each, %d engine steps, %zu raw bytes a frame\n", n_known, steps, raw_bytes);

  double shown[7];
  memcpy(shown, pose0, sizeof(pose0));
  for (int k = 0; k < steps; ++k) {
    pose_at((k + 1) * prm.delta_t, shown);
    if (render(shown)) return 1;
    CHECK(sl2_dev_upload(0, d_frames + NS * fb, &frames[NS * fb], fb));                 // the control's frame, as it is
    CHECK(sl2_convert_frames(conv, sl2_get_stream(eng), raw.data(), raw_bytes, /*raw_on_device=*/0, d_frames, fb));
    CHECK(sl2_go_one_step(eng, d_frames, fb, /*frames_on_device=*/1, /*save_trajectory=*/0, /*enable_mapping=*/0));
    CHECK(sl2_synchronize(eng));                        // (the raw buffer and the device frames are written again next step)
  }

  int32_t flags[B], got_filter[NS];
  sl2_frame_source got[NS];
  CHECK(sl2_get_status_flags(eng, 0, B, flags));
  CHECK(sl2_converter_get_sources(conv, 0, NS, got));
  CHECK(sl2_converter_get_filters(conv, 0, NS, got_filter));
  for (int b = 0; b < B; ++b) {
    double state[13], P[169];
    int32_t labels[32], counters[3];
    CHECK(sl2_get_vehicle_state(eng, b, 1, state, P));
    CHECK(sl2_get_selection(eng, b, labels, 32, counters));
    const double ex = state[0] - shown[0], ey = state[1] - shown[1], ez = state[2] - shown[2];
    const double err = std::sqrt(ex * ex + ey * ey + ez * ez);
    const sl2_camera& cam = b < NS ? scaled[cam_of[b]] : eng_cam;
    if (b < NS)
      printf("sequence %d  source %dx%d %s  filter %s  ", b, got[b].width, got[b].height, format_name(got[b].format), kFilterName[got_filter[b]]);
    else
      printf("sequence %d  source %dx%d %s  filter %s  ", b, eng_cam.width, eng_cam.height, "GRAY8", "NONE");
    printf("fku %.6f fkv %.6f u0 %.6f v0 %.6f kd1 %.6e sd %d  position error %.6f m  visible %d  selected %d  measured %d  flags %d\n", cam.fku, cam.fkv,
           cam.u0, cam.v0, cam.kd1, cam.sd, err, counters[0], counters[1], counters[2], flags[b]);
  }
  sl2_converter_destroy(conv);
  sl2_dev_free(0, d_grey); sl2_dev_free(0, d_pose); sl2_dev_free(0, d_origin); sl2_dev_free(0, d_tex);
  sl2_dev_free(0, d_frames);
  sl2_destroy(eng);
  return 0;
}
