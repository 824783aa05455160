// DenseSLAMSystem::traceSegments (se_hip_trace_segments_host) against the host se::Octree that getMap() builds from the same device map:
// segment for segment with se::geometry::trace_walk (include/se/segment_trace.hpp), every output, for both stop_at values, with all outputs
// and with status alone; a sample of short segments also against the literal definition.  And DenseSLAMSystem::segmentOf on random metric
// endpoints, written out for the Python rule to be held against.
//   usage: trace_mirror <scene.raw> <poses.bin> <volume_res> <volume_dim> <mu> <segments.bin>
// segments.bin receives, per endpoint pair, six float32 (a xyz, b xyz in metres) and the six int32 of segmentOf.
// Prints one line: "checked <n> occupied <n> unseen <n> empty <n> blocked <n> free <n> gain <n> literal <n> pairs <n> bad <n>" (counts of the
// host answers with stop_at occupied: statuses, blocked / free, segments with a non-zero unseen count; literal = segments also held to the
// definition; pairs = endpoint pairs written).
#include "mirror_scene.hpp"
#include <se/segment_trace.hpp>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <type_traits>
#include <vector>

int main(int argc, char** argv) {
  MirrorScene scene;
  if (int rc = scene.replay(argc, argv, 7, "scene.raw poses.bin res dim mu segments.bin")) return rc;
  DenseSLAMSystem& pipeline = *scene.pipeline;
  const int res = scene.res, S = 16 * res;
  std::shared_ptr<se::Octree<FieldType> > map;
  pipeline.getMap(map);
  if (map->getBlockBuffer().empty()) { std::fprintf(stderr, "empty map\n"); return 3; }

  const bool ofusion = std::is_same<FieldType, OFusion>::value;
  const se_hip_collide_test test = {0.f, ofusion ? 1 : 0};
  const se::geometry::voxel_test<FieldType> host_test = {0.f, ofusion};
  std::mt19937 rng(31);
  std::vector<int32_t> segs;
  auto add = [&](int ax, int ay, int az, int bx, int by, int bz) {
    const int32_t v[6] = {ax, ay, az, bx, by, bz};
    segs.insert(segs.end(), v, v + 6);
  };
  auto coord = [&]() { return (int)(rng() % (unsigned)(S + 800)) - 400; };
  auto span = [&](int m) { return (int)(rng() % (unsigned)(2 * m + 1)) - m; };
  // uniform (some start or end outside), then short ones around allocated blocks, where the surfaces are, then long ones
  for (int i = 0; i < 600; ++i) add(coord(), coord(), coord(), coord(), coord(), coord());
  const auto& blocks = map->getBlockBuffer();
  const size_t first_short = segs.size() / 6, n_short = 400;
  for (int i = 0; i < 1200; ++i) {
    const int* c = blocks[rng() % blocks.size()]->coordinates();
    const int m = (size_t)i < n_short ? 160 : 900;
    int a[3], b[3];
    for (int k = 0; k < 3; ++k) {
      a[k] = 16 * c[k] + span(200);
      if (i % 4 == 1) a[k] = a[k] / 16 * 16;                       // voxel corners
      b[k] = a[k] + (i % 4 == 1 ? 16 * span(m / 16) : span(m));
    }
    if (i % 9 == 0) b[i % 3] = a[i % 3];                            // planar, some of them in a grid plane
    add(a[0], a[1], a[2], b[0], b[1], b[2]);
  }
  add(8, 8, 8, S - 8, S - 8, S - 8);
  add(S, 0, S, 0, S, 0);
  add(-(1 << 22), S / 2 + 3, S / 2 + 5, 1 << 22, S / 2 + 3, S / 2 + 5);
  add(-400, -400, -400, -100, -90, -80);
  add((1 << 22) + 1, 0, 0, 0, 0, 0);                                // invalid
  add(0, 0, -(1 << 30), 5, 5, 5);                                   // invalid
  const size_t n = segs.size() / 6;

  long cnt[3] = {0, 0, 0}, blocked = 0, free_ = 0, gain = 0, literal = 0, bad = 0;
  for (int s = 0; s < 2; ++s) {
    const int32_t stop = s ? SE_HIP_COLLISION_UNSEEN : SE_HIP_COLLISION_OCCUPIED;
    const se::geometry::collision_status host_stop = s ? se::geometry::collision_status::unseen : se::geometry::collision_status::occupied;
    std::vector<uint8_t> status(n), status_only(n);
    std::vector<float> t_first(n), t_jump(n);
    std::vector<int32_t> first(3 * n), first_jump(3 * n), counts(2 * n);
    se_hip_trace_out out = {status.data(), t_first.data(), first.data(), counts.data()};
    if (!pipeline.traceSegments(segs.data(), n, test, stop, out)) { std::fprintf(stderr, "traceSegments failed\n"); return 4; }
    se_hip_trace_out out1 = {status_only.data(), t_jump.data(), first_jump.data(), nullptr};   // without counts: the jump instantiation
    if (!pipeline.traceSegments(segs.data(), n, test, stop, out1)) { std::fprintf(stderr, "traceSegments failed\n"); return 4; }
    for (size_t i = 0; i < n; ++i) {
      const int32_t* g = &segs[6 * i];
      const se::geometry::trace_result r = se::geometry::trace_walk(*map, g, host_test, host_stop);
      const int st = r.valid ? (int)r.status : SE_HIP_COLLISION_INVALID;
      const float t = se::geometry::to_float(r.t_first);
      bool same = st == (int)status[i] && st == (int)status_only[i] && std::memcmp(&t, &t_first[i], 4) == 0 && std::memcmp(&t, &t_jump[i], 4) == 0 &&
                  counts[2 * i] == r.unseen && counts[2 * i + 1] == r.empty;
      for (int k = 0; k < 3; ++k) same = same && first[3 * i + k] == r.first[k] && first_jump[3 * i + k] == r.first[k];
      if (i >= first_short && i < first_short + n_short) {
        const se::geometry::trace_result q = se::geometry::trace_literal(*map, g, host_test, host_stop);
        same = same && q.valid == r.valid && q.status == r.status && q.t_first.num == r.t_first.num && q.t_first.den == r.t_first.den && q.unseen == r.unseen &&
               q.empty == r.empty && q.first[0] == r.first[0] && q.first[1] == r.first[1] && q.first[2] == r.first[2];
        literal += s == 0;
      }
      if (!same) {
        if (bad < 5)
          std::fprintf(stderr, "segment %zu (%d %d %d | %d %d %d) stop_at %d: host %d %g (%d %d %d) %d %d, device %d %g (%d %d %d) %d %d, without counts %d %g (%d %d %d)\n", i,
                       g[0], g[1], g[2], g[3], g[4], g[5], (int)stop, st, (double)t, r.first[0], r.first[1], r.first[2], r.unseen, r.empty, (int)status[i],
                       (double)t_first[i], first[3 * i], first[3 * i + 1], first[3 * i + 2], counts[2 * i], counts[2 * i + 1], (int)status_only[i], (double)t_jump[i],
                       first_jump[3 * i], first_jump[3 * i + 1], first_jump[3 * i + 2]);
        ++bad;
      }
      if (s == 0 && r.valid) {
        ++cnt[st];
        if (t < 1.5f) ++blocked; else ++free_;
        if (r.unseen > 0) ++gain;
      }
    }
  }

  // segmentOf on metric endpoints around and beyond the volume, some on voxel boundaries
  FILE* f = std::fopen(argv[6], "wb");
  if (!f) { std::fprintf(stderr, "cannot write %s\n", argv[6]); return 2; }
  std::uniform_real_distribution<float> u(-1.f, scene.dim + 1.f);
  long pairs = 0;
  for (int i = 0; i < 2000; ++i, ++pairs) {
    float m[6];
    for (int k = 0; k < 6; ++k) m[k] = i % 5 == 0 ? (float)(int)(u(rng) * 40.f) * scene.dim / (float)res : u(rng);
    if (i % 7 == 0) { m[4] = m[1]; m[5] = m[2]; }
    int32_t sg[6];
    pipeline.segmentOf(Eigen::Vector3f(m[0], m[1], m[2]), Eigen::Vector3f(m[3], m[4], m[5]), sg);
    std::fwrite(m, 4, 6, f);
    std::fwrite(sg, 4, 6, f);
  }
  std::fclose(f);

  std::printf("checked %zu occupied %ld unseen %ld empty %ld blocked %ld free %ld gain %ld literal %ld pairs %ld bad %ld\n", n, cnt[0], cnt[1], cnt[2], blocked, free_, gain,
              literal, pairs, bad);
  return 0;
}
