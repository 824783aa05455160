// DenseSLAMSystem::castRays (se_hip_cast_rays_host) through the C++ mirror: drives it over a SLAMBench .raw stream with ground-truth
// poses, the way examples/denseslam_raw.cpp does, then casts the rays of rays.bin ([n][8] float32) and writes hit [n][4], normal [n][3]
// (float32) and status [n] (uint8) to out.bin, for tests/test_gpu_ray_cast.py to compare with the Python paths.
//   usage: ray_cast_mirror <scene.raw> <poses.bin> <volume_res> <volume_dim> <mu> <rays.bin> <out.bin>
// Prints one line: "rays <n> hits <n>".
#ifndef SE_FIELD_TYPE
#define SE_FIELD_TYPE SDF
#endif
#include <se/DenseSLAMSystem.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

int main(int argc, char** argv) {
  if (argc < 8) { std::fprintf(stderr, "usage: %s scene.raw poses.bin res dim mu rays.bin out.bin\n", argv[0]); return 2; }
  FILE* raw = std::fopen(argv[1], "rb");
  FILE* pf = std::fopen(argv[2], "rb");
  if (!raw || !pf) { std::fprintf(stderr, "cannot open inputs\n"); return 2; }
  const int res = std::atoi(argv[3]);
  const float dim = (float)std::atof(argv[4]), mu = (float)std::atof(argv[5]);
  uint32_t wh[2];
  if (std::fread(wh, 4, 2, raw) != 2) return 2;
  std::fseek(raw, 0, SEEK_SET);
  const int W = (int)wh[0], H = (int)wh[1];
  const Eigen::Vector4f k(481.2f * W / 640.f, 480.f * W / 640.f, 320.f * W / 640.f, 240.f * W / 640.f);
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
  DenseSLAMSystem pipeline(Eigen::Vector2i(W, H), Eigen::Vector3i(res, res, res), Eigen::Vector3f(dim, dim, dim),
                           Eigen::Vector3f(0.f, 0.f, 0.f), pyramid, config);
  std::vector<unsigned short> depth((size_t)W * H);
  std::vector<unsigned char> rgb((size_t)W * H * 3);
  float pose_rm[16];
  unsigned frame = 0;
  while (std::fread(wh, 4, 2, raw) == 2) {
    if (std::fread(depth.data(), 2, depth.size(), raw) != depth.size()) break;
    if (std::fread(wh, 4, 2, raw) != 2 || std::fread(rgb.data(), 1, rgb.size(), raw) != rgb.size()) break;
    if (std::fread(pose_rm, 4, 16, pf) != 16) break;
    Eigen::Matrix4f pose;
    for (int r = 0; r < 4; ++r)
      for (int c = 0; c < 4; ++c) pose(r, c) = pose_rm[r * 4 + c];
    pipeline.preprocessing(depth.data(), Eigen::Vector2i(W, H), false);
    pipeline.setPose(pose);
    pipeline.integration(k, 1, mu, frame);
    pipeline.raycasting(k, mu, frame);
    ++frame;
  }
  FILE* rf = std::fopen(argv[6], "rb");
  if (!rf) { std::fprintf(stderr, "cannot open rays\n"); return 2; }
  std::vector<float> rays;
  float r8[8];
  while (std::fread(r8, 4, 8, rf) == 8) rays.insert(rays.end(), r8, r8 + 8);
  std::fclose(rf);
  const size_t n = rays.size() / 8;
  std::vector<float> hit(4 * n), normal(3 * n);
  std::vector<uint8_t> status(n);
  se_hip_ray_out out{hit.data(), normal.data(), status.data()};
  if (!pipeline.castRays(rays.data(), n, mu, out)) return 4;
  FILE* of = std::fopen(argv[7], "wb");
  if (!of) return 2;
  std::fwrite(hit.data(), 4, hit.size(), of);
  std::fwrite(normal.data(), 4, normal.size(), of);
  std::fwrite(status.data(), 1, status.size(), of);
  std::fclose(of);
  size_t hits = 0;
  for (size_t i = 0; i < n; ++i) hits += (status[i] & SE_HIP_RAY_HIT) != 0;
  std::printf("rays %zu hits %zu\n", n, hits);
  return 0;
}
