// DenseSLAMSystem::shiftMap (se_hip_shift_map) on a live handle against se::shift_map (include/se/shift_map.hpp) applied to the getMap() snapshot
// taken before: a shift that drops part of the map, one by a single block, one that a side-64 node is aligned to, and one by the whole volume,
// one after the other, each compared octant by octant, value by value and flag by flag through a second getMap(), counts included; pose_ and
// init_pose_ move by exactly float(s) * voxel, getPosition() stays where it was to within the rounding of that addition.
// Drives the mirror over a SLAMBench .raw stream with ground-truth poses, the way examples/denseslam_raw.cpp does.
//   usage: shift_mirror <scene.raw> <poses.bin> <volume_res> <volume_dim> <mu>
// Prints one line: "shifts <n> kept <n> dropped <n> nodes_kept <n> nodes_dropped <n> left <n> bad <n>" (the counts summed over the shifts;
// left = blocks after the last one; bad = octants, values, flags, counts or pose components that differ from the host's).
#include "mirror_scene.hpp"
#include <se/shift_map.hpp>

#include <cmath>
#include <cstdio>
#include <cstring>

typedef se::Octree<FieldType> Map;

// octants, values or flags that differ between two snapshots
static long differing(Map& a, Map& b) {
  if (a.getBlockBuffer().size() != b.getBlockBuffer().size() || a.getNodesBuffer().size() != b.getNodesBuffer().size()) return 1;
  long d = 0;
  for (size_t i = 0; i < a.getBlockBuffer().size(); ++i) {
    auto &p = a.getBlockBuffer()[i], &q = b.getBlockBuffer()[i];
    if (p->code_ != q->code_ || p->active_ != q->active_ || std::memcmp(p->coordinates_, q->coordinates_, sizeof p->coordinates_)) { ++d; continue; }
    for (int v = 0; v < 512; ++v)
      if (std::memcmp(&p->voxel_block_[v].x, &q->voxel_block_[v].x, sizeof p->voxel_block_[v].x) || std::memcmp(&p->voxel_block_[v].y, &q->voxel_block_[v].y, sizeof p->voxel_block_[v].y)) ++d;
  }
  for (size_t i = 0; i < a.getNodesBuffer().size(); ++i) {
    auto &p = a.getNodesBuffer()[i], &q = b.getNodesBuffer()[i];
    if (p->code_ != q->code_ || p->side_ != q->side_) { ++d; continue; }
    for (int v = 0; v < 8; ++v)
      if (std::memcmp(&p->value_[v].x, &q->value_[v].x, sizeof p->value_[v].x) || std::memcmp(&p->value_[v].y, &q->value_[v].y, sizeof p->value_[v].y)) ++d;
  }
  return d;
}

int main(int argc, char** argv) {
  MirrorScene scene;
  if (int rc = scene.replay(argc, argv, 6, "scene.raw poses.bin res dim mu")) return rc;
  DenseSLAMSystem& pipeline = *scene.pipeline;
  const int res = scene.res;
  const float voxel = scene.dim / res;
  const int shifts[5][3] = {{-64, 0, 32}, {8, -8, 0}, {0, 64, 0}, {0, 0, 0}, {res, 0, 0}};
  long bad = 0;
  long long sum[4] = {0, 0, 0, 0};
  size_t left = 0;
  for (const auto& s : shifts) {
    std::shared_ptr<Map> before, after;
    pipeline.getMap(before);
    const Eigen::Matrix4f pose = pipeline.getPose();
    const Eigen::Vector3f init = pipeline.getInitPos(), position = pipeline.getPosition();
    int64_t dev[4] = {-1, -1, -1, -1}, host[4];
    if (!pipeline.shiftMap(Eigen::Vector3i(s[0], s[1], s[2]), dev)) { std::fprintf(stderr, "shiftMap failed\n"); return 4; }
    se::shift_map(*before, s, host);
    pipeline.getMap(after);
    const long d = differing(*before, *after);
    if (d != 0) { std::fprintf(stderr, "shift (%d, %d, %d): %ld octants / values / flags differ from the host's\n", s[0], s[1], s[2], d); bad += d; }
    for (int k = 0; k < 4; ++k) {
      if (dev[k] != host[k]) { std::fprintf(stderr, "counts[%d] device %lld host %lld\n", k, (long long)dev[k], (long long)host[k]); ++bad; }
      sum[k] += dev[k];
    }
    const Eigen::Matrix4f moved = pipeline.getPose();
    for (int k = 0; k < 3; ++k) {
      const float step = float(s[k]) * voxel;
      const float want_pose = pose(k, 3) + step, want_init = init(k) + step;
      const float got_pose = moved(k, 3), got_init = pipeline.getInitPos()(k);
      if (std::memcmp(&want_pose, &got_pose, 4) || std::memcmp(&want_init, &got_init, 4)) { std::fprintf(stderr, "pose_ / init_pose_ component %d\n", k); ++bad; }
      // pose_ + d and init_pose_ + d are each rounded once, so is their difference: three times half an ulp (2^-24 relative) of the largest
      const float mag = std::fmax(std::fmax(std::fabs(want_pose), std::fabs(want_init)), std::fabs(position(k)));
      if (std::fabs(pipeline.getPosition()(k) - position(k)) > std::ldexp(mag, -22)) { std::fprintf(stderr, "getPosition component %d\n", k); ++bad; }
    }
    for (int r = 0; r < 4; ++r)
      for (int c = 0; c < 3; ++c) if (moved(r, c) != pose(r, c)) ++bad;
    left = after->getBlockBuffer().size();
  }
  // a shift the library refuses leaves the pose alone
  const Eigen::Matrix4f pose = pipeline.getPose();
  if (pipeline.shiftMap(Eigen::Vector3i(4, 0, 0))) ++bad;
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) if (pipeline.getPose()(r, c) != pose(r, c)) ++bad;
  std::printf("shifts 5 kept %lld dropped %lld nodes_kept %lld nodes_dropped %lld left %zu bad %ld\n", sum[0], sum[1], sum[2], sum[3], left, bad);
  return 0;
}
