// The measuring half of tools/reach_bench.py: replays a scene into a live handle through the C++ mirror, then times, on that one map,
//   device   se_hip_reach_field with device output arrays (the call synchronises, so wall time around it is the call's cost), and its rounds
//   host     the route the library offered before: DenseSLAMSystem::getMap() once, then se::geometry::reach_field (a) per request
// and compares the two answers position for position.  One JSON line per variant on stdout.
//   usage: reach_bench <scene.raw> <poses.bin> <volume_res> <volume_dim> <mu> <map name> <reps> <sides, comma separated> [trace]
// trace: every device call once and nothing else (for `rocprofv3 --kernel-trace --stats`).
#include "../tests/cpp/mirror_scene.hpp"
#include <se/reach_field.hpp>

#include <hip/hip_runtime_api.h>

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

static double now_us() { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

int main(int argc, char** argv) {
  MirrorScene scene;
  if (int rc = scene.replay(argc, argv, 9, "scene.raw poses.bin res dim mu map reps sides [trace]")) return rc;
  DenseSLAMSystem& pipeline = *scene.pipeline;
  const int res = scene.res;
  const std::string map_name = argv[6];
  const int reps = std::atoi(argv[7]);
  std::vector<int> sides;
  for (char* t = std::strtok(argv[8], ","); t; t = std::strtok(nullptr, ",")) sides.push_back(std::atoi(t));
  const bool trace = argc > 9 && std::string(argv[9]) == "trace";
  se_hip_pipeline* h = pipeline.handle();
  se_hip_sync(h);

  // the host route's first share: the snapshot (twice; the second is the one kept)
  std::shared_ptr<se::Octree<FieldType> > map;
  double getmap_us[2] = {0, 0};
  for (int r = 0; r < 2; ++r) {
    map.reset();
    const double t0 = now_us();
    pipeline.getMap(map);
    getmap_us[r] = now_us() - t0;
  }
  const se_hip_collide_test test = {0.f, 0};
  const se::geometry::voxel_test<FieldType> host_test = {0.f, false};

  // placements: a raycast hit of the last frame; the centre of the 16^3 box, of 4096 placed uniformly, that is free and farthest from the hit
  std::vector<float> vertex((size_t)scene.W * scene.H * 3), normal((size_t)scene.W * scene.H * 3);
  if (se_hip_download_vertex_normal(h, vertex.data(), normal.data()) != 0) return 3;
  std::mt19937 rng(1);
  int surface[3] = {0, 0, 0}, open_space[3] = {0, 0, 0};
  for (int tries = 0; tries < 100000; ++tries) {
    const size_t px = rng() % ((size_t)scene.W * scene.H);
    if (normal[3 * px] == -2.f || !(vertex[3 * px] > 0.f && vertex[3 * px + 1] > 0.f && vertex[3 * px + 2] > 0.f)) continue;
    for (int k = 0; k < 3; ++k) surface[k] = (int)(vertex[3 * px + k] * (float)res / scene.dim);
    break;
  }
  {
    std::vector<int32_t> boxes;
    for (int i = 0; i < 4096; ++i) {
      for (int k = 0; k < 3; ++k) boxes.push_back(72 + (int)(rng() % (unsigned)(res - 160)));
      for (int k = 0; k < 3; ++k) boxes.push_back(16);
    }
    std::vector<uint8_t> status(4096);
    if (se_hip_collide_boxes_host(h, boxes.data(), 4096, &test, SE_HIP_COLLIDE_STRICT, status.data()) != 0) return 3;
    long best = -1;
    for (int i = 0; i < 4096; ++i) {
      if (status[i] != SE_HIP_COLLISION_EMPTY) continue;
      long d = 0;
      for (int k = 0; k < 3; ++k) { const long e = boxes[6 * i + k] + 8 - surface[k]; d += e * e; }
      if (d > best) { best = d; for (int k = 0; k < 3; ++k) open_space[k] = boxes[6 * i + k] + 8; }
    }
    if (best < 0) { std::fprintf(stderr, "no empty box\n"); return 3; }
  }

  for (const int side : sides) {
    const size_t count = (size_t)side * side * side;
    int32_t* d_steps = nullptr;
    uint8_t *d_seed = nullptr, *d_next = nullptr;
    if (hipMalloc((void**)&d_steps, count * 4) != hipSuccess || hipMalloc((void**)&d_seed, count) != hipSuccess || hipMalloc((void**)&d_next, count) != hipSuccess) return 4;
    std::vector<int32_t> steps(count);
    std::vector<uint8_t> seed(count), next(count);
    for (int place = 0; place < 2; ++place) {
      const int* centre = place ? open_space : surface;
      for (const int robot : {1, 4})
        for (const int n_seeds : {1, 16}) {
          se::geometry::reach_request q;
          for (int k = 0; k < 3; ++k) { q.lo(k) = centre[k] - side / 2; q.side(k) = side; q.robot(k) = robot; }
          // seeds: the region's centre, then positions spread over the region (the same for both routes; unusable ones are ignored by both)
          std::mt19937 srng(7u + (unsigned)side);
          q.seeds.push_back({{centre[0], centre[1], centre[2]}});
          for (int s = 1; s < n_seeds; ++s) q.seeds.push_back({{q.lo(0) + (int)(srng() % (unsigned)side), q.lo(1) + (int)(srng() % (unsigned)side), q.lo(2) + (int)(srng() % (unsigned)side)}});
          std::vector<int32_t> flat;
          for (const se::geometry::int3& p : q.seeds)
            for (int k = 0; k < 3; ++k) flat.push_back(p(k));
          se_hip_reach_request rq;
          for (int k = 0; k < 3; ++k) { rq.lo[k] = q.lo(k); rq.side[k] = side; rq.robot[k] = robot; }
          rq.stop_at = SE_HIP_COLLISION_OCCUPIED; rq.n_seeds = n_seeds; rq.seeds = flat.data();
          int64_t counts[4] = {0, 0, 0, 0};
          const se_hip_reach_out out = {d_steps, d_seed, d_next, counts};
          if (trace) {
            if (se_hip_reach_field(h, &rq, &test, &out) != 0) return 5;
            continue;
          }
          double device_us[2] = {0, 0}, host_us[2] = {0, 0};
          se::geometry::reach_result host;
          for (int run = 0; run < 2; ++run) {   // every variant twice, the routes alternating
            for (int r = -2; r < reps; ++r) {   // (two warm-up calls)
              const double t0 = now_us();
              if (se_hip_reach_field(h, &rq, &test, &out) != 0) { std::fprintf(stderr, "se_hip_reach_field: %s\n", se_hip_last_error()); return 5; }
              if (r >= 0) device_us[run] += (now_us() - t0) / reps;
            }
            const double t0 = now_us();
            if (!se::geometry::reach_field(*map, q, host_test, se::geometry::collision_status::occupied, host)) return 6;
            host_us[run] = now_us() - t0;
          }
          if (hipMemcpy(steps.data(), d_steps, count * 4, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(seed.data(), d_seed, count, hipMemcpyDeviceToHost) != hipSuccess ||
              hipMemcpy(next.data(), d_next, count, hipMemcpyDeviceToHost) != hipSuccess)
            return 4;
          const bool equal = steps == host.steps && seed == host.seed && next == host.next && counts[0] == host.counts[0] && counts[1] == host.counts[1] && counts[2] == host.counts[2];
          const double dev = (device_us[0] + device_us[1]) / 2, hst = (host_us[0] + host_us[1]) / 2, gm = (getmap_us[0] + getmap_us[1]) / 2;
          std::printf("{\"res\": %d, \"field\": \"sdf\", \"layout\": \"dense\", \"map\": \"%s\", \"place\": \"%s\", \"side\": %d, \"robot\": %d, \"seeds\": %d, "
                      "\"positions\": %zu, \"free\": %ld, \"reached\": %ld, \"max_steps\": %ld, \"rounds\": %ld, "
                      "\"device_us_per_call\": %.1f, \"device_us_runs\": [%.1f, %.1f], \"host_bfs_us\": %.1f, \"host_bfs_us_runs\": [%.1f, %.1f], "
                      "\"getmap_us\": %.1f, \"getmap_us_runs\": [%.1f, %.1f], \"host_over_device\": %.3f, \"host_with_getmap_over_device\": %.3f, \"equal\": %s}\n",
                      res, map_name.c_str(), place ? "free" : "surface", side, robot, n_seeds, count, (long)counts[0], (long)counts[1], (long)counts[2], (long)counts[3], dev,
                      device_us[0], device_us[1], hst, host_us[0], host_us[1], gm, getmap_us[0], getmap_us[1], hst / dev, (hst + gm) / dev, equal ? "true" : "false");
          std::fflush(stdout);
        }
    }
    (void)hipFree(d_steps); (void)hipFree(d_seed); (void)hipFree(d_next);
  }
  return 0;
}
