// DenseSLAMSystem::meshBlocks (se_hip_mesh_blocks_host) through the C++ mirror: drives it over a SLAMBench .raw stream with ground-truth
// poses, the way examples/denseslam_raw.cpp does, then meshes the blocks of the region lo / hi that the last `n_views` poses may have touched
// (0: the region alone) and writes header [4] int64, block_coords [B][3] int32, block_range [B][2] int64 and triangles [T][9] float32 to
// out.bin, for tests/test_gpu_live_mesh.py to compare with the Python paths.
//   usage: mesh_blocks_mirror <scene.raw> <poses.bin> <volume_res> <volume_dim> <mu> <n_views> <lo> <hi> <skip_empty> <out.bin>
// Prints one line: "blocks <B> triangles <T>".
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
  if (argc < 11) { std::fprintf(stderr, "usage: %s scene.raw poses.bin res dim mu n_views lo hi skip_empty out.bin\n", argv[0]); return 2; }
  FILE* raw = std::fopen(argv[1], "rb");
  FILE* pf = std::fopen(argv[2], "rb");
  if (!raw || !pf) { std::fprintf(stderr, "cannot open inputs\n"); return 2; }
  const int res = std::atoi(argv[3]);
  const float dim = (float)std::atof(argv[4]), mu = (float)std::atof(argv[5]);
  const int n_views = std::atoi(argv[6]), lo = std::atoi(argv[7]), hi = std::atoi(argv[8]), skip = std::atoi(argv[9]);
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
  std::vector<se_hip_mesh_view> views;
  float pose_rm[16];
  unsigned frame = 0;
  while (std::fread(wh, 4, 2, raw) == 2) {
    if (std::fread(depth.data(), 2, depth.size(), raw) != depth.size()) break;
    if (std::fread(wh, 4, 2, raw) != 2 || std::fread(rgb.data(), 1, rgb.size(), raw) != rgb.size()) break;
    if (std::fread(pose_rm, 4, 16, pf) != 16) break;
    Eigen::Matrix4f pose;
    se_hip_mesh_view v;
    for (int r = 0; r < 4; ++r)
      for (int c = 0; c < 4; ++c) { pose(r, c) = pose_rm[r * 4 + c]; v.pose[c * 4 + r] = pose_rm[r * 4 + c]; }
    for (int i = 0; i < 4; ++i) v.k[i] = k(i);
    v.width = W; v.height = H;
    views.push_back(v);
    pipeline.preprocessing(depth.data(), Eigen::Vector2i(W, H), false);
    pipeline.setPose(pose);
    pipeline.integration(k, 1, mu, frame);
    pipeline.raycasting(k, mu, frame);
    ++frame;
  }
  if ((size_t)n_views > views.size()) return 2;
  se_hip_mesh_select sel;
  for (int i = 0; i < 3; ++i) { sel.lo[i] = lo; sel.hi[i] = hi; }
  sel.n_views = n_views; sel.flags = skip ? SE_HIP_MESH_SKIP_EMPTY : 0u;
  sel.views = n_views ? views.data() + (views.size() - (size_t)n_views) : nullptr;
  int64_t header[4] = {0, 0, 0, 0};
  se_hip_mesh_out out{nullptr, 0, nullptr, nullptr, 0, header};
  if (!pipeline.meshBlocks(sel, out)) return 4;   // the sizing call
  std::vector<float> tri((size_t)header[1] * 9);
  std::vector<int32_t> coords((size_t)header[0] * 3);
  std::vector<int64_t> range((size_t)header[0] * 2);
  out = se_hip_mesh_out{tri.data(), header[1], coords.data(), range.data(), header[0], header};
  if (header[0] && !pipeline.meshBlocks(sel, out)) return 4;
  FILE* of = std::fopen(argv[10], "wb");
  if (!of) return 2;
  std::fwrite(header, 8, 4, of);
  std::fwrite(coords.data(), 4, coords.size(), of);
  std::fwrite(range.data(), 8, range.size(), of);
  std::fwrite(tri.data(), 4, tri.size(), of);
  std::fclose(of);
  std::printf("blocks %lld triangles %lld\n", (long long)header[2], (long long)header[3]);
  return 0;
}
