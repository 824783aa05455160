// DenseSLAMSystem::castRays (se_hip_cast_rays_host) through the C++ mirror: drives it over a SLAMBench .raw stream with ground-truth
// poses, the way examples/denseslam_raw.cpp does, then casts the rays of rays.bin ([n][8] float32) and writes hit [n][4], normal [n][3]
// (float32) and status [n] (uint8) to out.bin, for tests/test_gpu_ray_cast.py to compare with the Python paths.
//   usage: ray_cast_mirror <scene.raw> <poses.bin> <volume_res> <volume_dim> <mu> <rays.bin> <out.bin>
// Prints one line: "rays <n> hits <n>".
#include "mirror_scene.hpp"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

int main(int argc, char** argv) {
  MirrorScene scene;
  if (int rc = scene.replay(argc, argv, 8, "scene.raw poses.bin res dim mu rays.bin out.bin")) return rc;
  DenseSLAMSystem& pipeline = *scene.pipeline;
  const float mu = scene.mu;
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
