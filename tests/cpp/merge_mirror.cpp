// DenseSLAMSystem::mergeMap (se_hip_merge_map) on two live handles against se::merge_map (include/se/merge_map.hpp) applied to their getMap()
// snapshots taken before: the three modes and shifts of 0, one unaligned to every node, one aligned to side-64 nodes and one that clips, one
// after the other into the same destination, each compared octant by octant, value by value and flag by flag through a second getMap(), counts
// included; the source's snapshot and the poses of both pipelines must not change.
// Drives two mirrors over two SLAMBench .raw streams with ground-truth poses (tests/cpp/mirror_scene.hpp).
//   usage: merge_mirror <dst.raw> <dst_poses.bin> <dst_res> <dst_dim> <mu> <src.raw> <src_poses.bin> <src_res> <src_dim>
// Prints one line: "merges <n> combined <n> created <n> clipped <n> nodes_combined <n> nodes_created <n> nodes_skipped <n> blocks <n> bad <n>"
// (the counts summed over the merges; blocks = the destination's after the last one; bad = octants, values, flags, counts or pose components
// that differ from the host's).
#include "mirror_scene.hpp"
#include <se/merge_map.hpp>

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
  if (argc < 10) { std::fprintf(stderr, "usage: %s dst.raw dst_poses.bin dst_res dst_dim mu src.raw src_poses.bin src_res src_dim\n", argv[0]); return 2; }
  MirrorScene dst_scene, src_scene;
  char* src_argv[6] = {argv[0], argv[6], argv[7], argv[8], argv[9], argv[5]};
  if (int rc = dst_scene.replay(6, argv, 6, "dst.raw dst_poses.bin dst_res dst_dim mu")) return rc;
  if (int rc = src_scene.replay(6, src_argv, 6, "src.raw src_poses.bin src_res src_dim mu")) return rc;
  DenseSLAMSystem& dst = *dst_scene.pipeline;
  DenseSLAMSystem& src = *src_scene.pipeline;
  struct Case { int s[3]; int mode; float max_weight; };
  const Case cases[6] = {{{8, 0, -16}, SE_HIP_MERGE_FILL, 100.f}, {{0, 0, 0}, SE_HIP_MERGE_FUSE, 100.f}, {{64, 0, 0}, SE_HIP_MERGE_REPLACE, 100.f},
                         {{-16, 16, 0}, SE_HIP_MERGE_FUSE, 7.f}, {{0, 0, 0}, SE_HIP_MERGE_FUSE, 255.f}, {{0, -32, 32}, SE_HIP_MERGE_FILL, 1.f}};
  long bad = 0;
  long long sum[6] = {0, 0, 0, 0, 0, 0};
  size_t blocks = 0;
  const Eigen::Matrix4f dst_pose = dst.getPose(), src_pose = src.getPose();
  for (const Case& c : cases) {
    std::shared_ptr<Map> before, source, after, source_after;
    dst.getMap(before);
    src.getMap(source);
    int64_t dev[12], host[12];
    for (int k = 0; k < 12; ++k) dev[k] = -7;
    const se_hip_merge_rule rule{c.mode, c.max_weight};
    if (!dst.mergeMap(src, Eigen::Vector3i(c.s[0], c.s[1], c.s[2]), rule, dev)) { std::fprintf(stderr, "mergeMap failed\n"); return 4; }
    se::merge_rule hr; hr.mode = c.mode; hr.max_weight = c.max_weight;
    se::merge_map(*before, *source, c.s, hr, host);
    dst.getMap(after);
    src.getMap(source_after);
    const long d = differing(*before, *after) + differing(*source, *source_after);
    if (d != 0) { std::fprintf(stderr, "merge (%d, %d, %d) mode %d: %ld octants / values / flags differ from the host's\n", c.s[0], c.s[1], c.s[2], c.mode, d); bad += d; }
    for (int k = 0; k < 12; ++k)
      if (dev[k] != host[k]) { std::fprintf(stderr, "counts[%d] device %lld host %lld\n", k, (long long)dev[k], (long long)host[k]); ++bad; }
    for (int k = 0; k < 6; ++k) sum[k] += dev[k];
    blocks = after->getBlockBuffer().size();
  }
  // a merge the library refuses (into itself; a shift that is no multiple of 8) reports failure, and no merge moves a pose
  if (dst.mergeMap(dst)) ++bad;
  if (dst.mergeMap(src, Eigen::Vector3i(4, 0, 0))) ++bad;
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) if (dst.getPose()(r, c) != dst_pose(r, c) || src.getPose()(r, c) != src_pose(r, c)) ++bad;
  std::printf("merges 6 combined %lld created %lld clipped %lld nodes_combined %lld nodes_created %lld nodes_skipped %lld blocks %zu bad %ld\n",
              sum[0], sum[1], sum[2], sum[3], sum[4], sum[5], blocks, bad);
  return 0;
}
