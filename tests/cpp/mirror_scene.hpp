// The scene driver the *_mirror.cpp programs share: it runs the C++ mirror (include/se/DenseSLAMSystem.h) over a SLAMBench .raw stream with
// ground-truth poses, the way examples/denseslam_raw.cpp does, and hands the live pipeline to the program.
//   arguments: <scene.raw> <poses.bin> <volume_res> <volume_dim> <mu> [the program's own ...]
// poses.bin holds one row-major float32 4x4 camera-to-world pose per frame; the intrinsics are (481.2, 480, 320, 240) * W / 640.
#ifndef SE_TESTS_MIRROR_SCENE_HPP
#define SE_TESTS_MIRROR_SCENE_HPP
#ifndef SE_FIELD_TYPE
#define SE_FIELD_TYPE SDF
#endif
#include <se/DenseSLAMSystem.h>

#include <cstdio>
#include <cstdlib>
#include <functional>
#include <memory>
#include <vector>

struct MirrorScene {
  int W = 0, H = 0, res = 0;
  float dim = 0.f, mu = 0.f;
  Eigen::Vector4f k;
  unsigned frames = 0;   // frames replayed
  std::unique_ptr<DenseSLAMSystem> pipeline;

  // called once per frame, before the frame is integrated: frame index, the row-major pose, k
  typedef std::function<void(unsigned, const float*, const Eigen::Vector4f&)> FrameHook;

  // preprocessing -> setPose -> integration -> raycasting per frame.  Returns 0, or the exit code (2: bad arguments or unopenable inputs,
  // after the message on stderr); `usage` names the arguments after the program's name, of which there must be min_argc - 1.
  int replay(int argc, char** argv, int min_argc, const char* usage, const FrameHook& each_frame = FrameHook()) {
    if (argc < min_argc) { std::fprintf(stderr, "usage: %s %s\n", argv[0], usage); return 2; }
    FILE* raw = std::fopen(argv[1], "rb");
    FILE* pf = std::fopen(argv[2], "rb");
    if (!raw || !pf) { std::fprintf(stderr, "cannot open inputs\n"); return 2; }
    res = std::atoi(argv[3]);
    dim = (float)std::atof(argv[4]); mu = (float)std::atof(argv[5]);
    uint32_t wh[2];
    if (std::fread(wh, 4, 2, raw) != 2) return 2;
    std::fseek(raw, 0, SEEK_SET);
    W = (int)wh[0]; H = (int)wh[1];
    k = Eigen::Vector4f(481.2f * W / 640.f, 480.f * W / 640.f, 320.f * W / 640.f, 240.f * W / 640.f);
    std::vector<int> pyramid = {10, 5, 4};
    Configuration config;
    config.compute_size_ratio = 1; config.tracking_rate = 1; config.integration_rate = 1; config.rendering_rate = 4;
    config.volume_resolution = Eigen::Vector3i(res, res, res); config.volume_size = Eigen::Vector3f(dim, dim, dim);
    config.initial_pos_factor = Eigen::Vector3f(0.f, 0.f, 0.f); config.pyramid = pyramid;
    config.dump_volume_file = ""; config.input_file = argv[1]; config.log_file = ""; config.groundtruth_file = argv[2];
    config.gt_transform = Eigen::Matrix4f::Identity(); config.camera = k; config.camera_overrided = false;
    config.mu = mu; config.fps = 0; config.blocking_read = false; config.icp_threshold = 1e-5f; config.no_gui = true;
    config.render_volume_fullsize = false; config.bilateralFilter = false;
    config.colouredVoxels = false; config.multiResolution = false; config.bayesian = false;
    pipeline.reset(new DenseSLAMSystem(Eigen::Vector2i(W, H), Eigen::Vector3i(res, res, res), Eigen::Vector3f(dim, dim, dim),
                                       Eigen::Vector3f(0.f, 0.f, 0.f), pyramid, config));
    std::vector<unsigned short> depth((size_t)W * H);
    std::vector<unsigned char> rgb((size_t)W * H * 3);
    float pose_rm[16];
    frames = 0;
    while (std::fread(wh, 4, 2, raw) == 2) {
      if (std::fread(depth.data(), 2, depth.size(), raw) != depth.size()) break;
      if (std::fread(wh, 4, 2, raw) != 2 || std::fread(rgb.data(), 1, rgb.size(), raw) != rgb.size()) break;
      if (std::fread(pose_rm, 4, 16, pf) != 16) break;
      Eigen::Matrix4f pose;
      for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) pose(r, c) = pose_rm[r * 4 + c];
      if (each_frame) each_frame(frames, pose_rm, k);
      pipeline->preprocessing(depth.data(), Eigen::Vector2i(W, H), false);
      pipeline->setPose(pose);
      pipeline->integration(k, 1, mu, frames);
      pipeline->raycasting(k, mu, frames);
      ++frames;
    }
    std::fclose(raw);
    std::fclose(pf);
    return 0;
  }
};

#endif /* SE_TESTS_MIRROR_SCENE_HPP */
