// DenseSLAMSystem::meshBlocks (se_hip_mesh_blocks_host) through the C++ mirror: drives it over a SLAMBench .raw stream with ground-truth
// poses, the way examples/denseslam_raw.cpp does, then meshes the blocks of the region lo / hi that the last `n_views` poses may have touched
// (0: the region alone) and writes header [4] int64, block_coords [B][3] int32, block_range [B][2] int64 and triangles [T][9] float32 to
// out.bin, for tests/test_gpu_live_mesh.py to compare with the Python paths.
//   usage: mesh_blocks_mirror <scene.raw> <poses.bin> <volume_res> <volume_dim> <mu> <n_views> <lo> <hi> <skip_empty> <out.bin>
// Prints one line: "blocks <B> triangles <T>".
#include "mirror_scene.hpp"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

int main(int argc, char** argv) {
  std::vector<se_hip_mesh_view> views;
  MirrorScene scene;
  const int rc = scene.replay(argc, argv, 11, "scene.raw poses.bin res dim mu n_views lo hi skip_empty out.bin", [&](unsigned, const float* pose_rm, const Eigen::Vector4f& k) {
    se_hip_mesh_view v;
    for (int r = 0; r < 4; ++r)
      for (int c = 0; c < 4; ++c) v.pose[c * 4 + r] = pose_rm[r * 4 + c];
    for (int i = 0; i < 4; ++i) v.k[i] = k(i);
    v.width = scene.W; v.height = scene.H;
    views.push_back(v);
  });
  if (rc) return rc;
  DenseSLAMSystem& pipeline = *scene.pipeline;
  const int n_views = std::atoi(argv[6]), lo = std::atoi(argv[7]), hi = std::atoi(argv[8]), skip = std::atoi(argv[9]);
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
