// The host half of tools/trace_bench.py: replays a scene into a live handle through the C++ mirror, takes the getMap() snapshot (timed, twice)
// and times se::geometry::trace_walk (include/se/segment_trace.hpp) -- with counts, and without (the jumps) -- over segment sets read from
// files, on one thread; the answers are compared with DenseSLAMSystem::traceSegments on the same map.  One JSON line per set on stdout.
//   usage: trace_bench <scene.raw> <poses.bin> <volume_res> <volume_dim> <mu> <host segments per set> <name>=<segments.bin> ...
// A segments file holds int32 [n][6]; of a set the first <host segments per set> are walked on the host.
#include "../tests/cpp/mirror_scene.hpp"
#include <se/segment_trace.hpp>

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

static double now_us() { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

int main(int argc, char** argv) {
  MirrorScene scene;
  if (int rc = scene.replay(argc, argv, 8, "scene.raw poses.bin res dim mu host_segments name=segments.bin ...")) return rc;
  DenseSLAMSystem& pipeline = *scene.pipeline;
  const size_t host_cap = (size_t)std::atol(argv[6]);
  se_hip_sync(pipeline.handle());
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
  const se::geometry::collision_status stop = se::geometry::collision_status::occupied;
  for (int a = 7; a < argc; ++a) {
    const std::string arg = argv[a];
    const size_t eq = arg.find('=');
    if (eq == std::string::npos) { std::fprintf(stderr, "expected name=file, got %s\n", argv[a]); return 2; }
    FILE* f = std::fopen(arg.substr(eq + 1).c_str(), "rb");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", arg.substr(eq + 1).c_str()); return 2; }
    std::vector<int32_t> segs;
    int32_t buf[6];
    while (std::fread(buf, 4, 6, f) == 6) segs.insert(segs.end(), buf, buf + 6);
    std::fclose(f);
    const size_t n = std::min(segs.size() / 6, host_cap);
    std::vector<uint8_t> status(n);
    std::vector<float> t_first(n);
    std::vector<int32_t> first(3 * n), counts(2 * n);
    se_hip_trace_out out = {status.data(), t_first.data(), first.data(), counts.data()};
    if (!pipeline.traceSegments(segs.data(), n, test, SE_HIP_COLLISION_OCCUPIED, out)) return 4;
    double walk_us[2] = {0, 0};
    long differ = 0, steps = 0;
    for (int mode = 0; mode < 2; ++mode) {
      const double t0 = now_us();
      for (size_t i = 0; i < n; ++i) {
        const se::geometry::trace_result r = se::geometry::trace_walk(*map, &segs[6 * i], host_test, stop, mode == 0);
        const float t = se::geometry::to_float(r.t_first);
        const int st = r.valid ? (int)r.status : SE_HIP_COLLISION_INVALID;
        bool same = st == (int)status[i] && std::memcmp(&t, &t_first[i], 4) == 0 && first[3 * i] == r.first[0] && first[3 * i + 1] == r.first[1] && first[3 * i + 2] == r.first[2];
        if (mode == 0) { same = same && counts[2 * i] == r.unseen && counts[2 * i + 1] == r.empty; steps += r.valid ? r.unseen + r.empty : 0; }
        differ += same ? 0 : 1;
      }
      walk_us[mode] = now_us() - t0;
    }
    std::printf("{\"set\": \"%s\", \"host_segments\": %zu, \"getmap_us\": [%.0f, %.0f], \"walk_us\": %.0f, \"walk_nocount_us\": %.0f, \"counted_voxels\": %ld, \"differ\": %ld}\n",
                arg.substr(0, eq).c_str(), n, getmap_us[0], getmap_us[1], walk_us[0], walk_us[1], steps, differ);
    std::fflush(stdout);
  }
  return 0;
}
