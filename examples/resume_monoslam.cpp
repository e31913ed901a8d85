// Stop a run and continue it in another object: the loop of examples/monoslam_adapter.cpp, interrupted after --save-at frames by
// MonoSLAM::SaveState(file); a NEW MonoSLAM is then initialised from the same configuration, LoadState(file) replaces its map,
// and the remaining frames follow.  The standard output is line for line what monoslam_adapter prints for the uninterrupted run
// (tests/test_gpu_checkpoint.py compares the two); what concerns the interruption goes to the standard error.
//
//   resume_monoslam --cfg scene.cfg --frames frame_dir [--mapping] [--save-at k] [--state file]
#include <scenelib2_amd_monoslam.hpp>

#include <cstdio>
#include <memory>

int main(int argc, char** argv) {
  std::string cfg, frames_dir, state = "resume_monoslam.state";
  bool enable_mapping = false;
  int save_at = -1;
  for (int i = 1; i < argc; ++i) {
    const std::string a = argv[i];
    if (a == "--cfg" && i + 1 < argc) cfg = argv[++i];
    else if (a == "--frames" && i + 1 < argc) frames_dir = argv[++i];
    else if (a == "--state" && i + 1 < argc) state = argv[++i];
    else if (a == "--save-at" && i + 1 < argc) save_at = std::atoi(argv[++i]);
    else if (a == "--mapping") enable_mapping = true;
    else { fprintf(stderr, "usage: %s --cfg scene.cfg --frames dir [--mapping] [--save-at k] [--state file]\n", argv[0]); return 2; }
  }
  if (cfg.empty() || frames_dir.empty()) { fprintf(stderr, "need --cfg and --frames\n"); return 2; }
  try {
    std::unique_ptr<SceneLib2Amd::MonoSLAM> slam(new SceneLib2Amd::MonoSLAM());
    slam->Init(cfg);
    printf("camera %dx%d, %zu known features\n", slam->camera_->width_, slam->camera_->height_, slam->feature_list_.size());
    const char* dirs[1] = {frames_dir.c_str()};
    const int width = slam->camera_->width_, height = slam->camera_->height_;
    sl2_ingest* grab = nullptr;
    if (sl2_ingest_open(dirs, 1, width, height, 0, 8, &grab) != SL2_OK) { fprintf(stderr, "%s\n", sl2_last_error()); return 1; }
    const int n = sl2_ingest_frame_count(grab);
    if (save_at < 0) save_at = n / 2;
    for (int frame_id = 0; frame_id < n; ++frame_id) {
      if (frame_id == save_at) {
        slam->SaveState(state);
        fprintf(stderr, "saved after %d frames: %zu features, %zu partially initialised\n", frame_id, slam->feature_list_.size(),
                slam->feature_init_info_vector_.size());
        // a later process would start here: a new object and a new grabber positioned at the next frame
        sl2_ingest_close(grab);
        slam.reset(new SceneLib2Amd::MonoSLAM());
        slam->Init(cfg);
        slam->LoadState(state);
        if (sl2_ingest_open(dirs, 1, width, height, 0, 8, &grab) != SL2_OK) { fprintf(stderr, "%s\n", sl2_last_error()); return 1; }
        for (int skip = 0; skip < frame_id; ++skip) {
          const uint8_t* unused = nullptr;
          size_t stride = 0;
          if (sl2_ingest_next(grab, slam->stream(), &unused, &stride) != SL2_OK) { fprintf(stderr, "%s\n", sl2_last_error()); return 1; }
        }
        fprintf(stderr, "restored: %zu features, %zu partially initialised\n", slam->feature_list_.size(), slam->feature_init_info_vector_.size());
      }
      SceneLib2Amd::Frame frame;
      size_t stride = 0;
      if (sl2_ingest_next(grab, slam->stream(), &frame.data, &stride) != SL2_OK) { fprintf(stderr, "%s\n", sl2_last_error()); return 1; }
      frame.cols = width; frame.rows = height; frame.on_device = true;
      slam->GoOneStep(frame, true, enable_mapping);
      if (frame_id % 10 == 9 || frame_id + 1 == n) {
        int measured = 0;
        for (const SceneLib2Amd::Feature* f : slam->selected_feature_list_) measured += f->successful_measurement_flag_ ? 1 : 0;
        printf("frame %4d  r = (% .4f % .4f % .4f)  features %zu  visible %d  selected %zu  measured %d  partial %zu\n", frame_id,
               slam->xv_[0], slam->xv_[1], slam->xv_[2], slam->feature_list_.size(), slam->number_of_visible_features_,
               slam->selected_feature_list_.size(), measured, slam->feature_init_info_vector_.size());
      }
    }
    sl2_ingest_close(grab);
    slam->print_robot_state();
  } catch (const std::exception& e) {
    fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
