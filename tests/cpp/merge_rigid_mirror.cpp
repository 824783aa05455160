// DenseSLAMSystem::mergeMapRigid (se_hip_merge_map_rigid) on two live handles against se::merge_map_rigid (include/se/merge_rigid.hpp) applied to
// their getMap() snapshots taken before, with the pull transform of DenseSLAMSystem::rigidPull: `yaw` (30 degrees about the vertical, a
// fractional translation) and `quarter` (90 degrees about z, a translation by whole voxels), one after the other into the same destination, each
// compared octant by octant, value by value and flag by flag through a second getMap(), counts included; the source's snapshot and the poses of
// both pipelines must not change.
// Drives two mirrors over two SLAMBench .raw streams with ground-truth poses (tests/cpp/mirror_scene.hpp).
//   usage: merge_rigid_mirror <dst.raw> <dst_poses.bin> <dst_res> <dst_dim> <mu> <src.raw> <src_poses.bin> <src_res> <src_dim>
// Prints one line: "merges <n> combined <n> created <n> observed <n> both <n> blocks <n> bad <n>" (the counts summed over the merges; blocks =
// the destination's after the last one; bad = octants, values, flags, counts or pose components that differ from the host's).
#include "mirror_scene.hpp"
#include <se/merge_rigid.hpp>

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

// the metric pose that turns by R about the source's centre and carries it to the destination's centre plus `extra` voxels
static Eigen::Matrix4f about_centres(const double R[3][3], int src_res, int dst_res, double voxel, const double extra[3], bool whole) {
  Eigen::Matrix4f T;
  for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) T(r, c) = r == c ? 1.f : 0.f;
  const double cs = (src_res - 1) / 2.0, cd = (dst_res - src_res) / 2 + (src_res - 1) / 2.0;
  for (int r = 0; r < 3; ++r) {
    double t = cd + extra[r];
    for (int c = 0; c < 3; ++c) { T(r, c) = (float)R[r][c]; t -= R[r][c] * cs; }
    if (whole) t = std::floor(t);
    T(r, 3) = (float)(t * voxel);
  }
  return T;
}

int main(int argc, char** argv) {
  if (argc < 10) { std::fprintf(stderr, "usage: %s dst.raw dst_poses.bin dst_res dst_dim mu src.raw src_poses.bin src_res src_dim\n", argv[0]); return 2; }
  MirrorScene dst_scene, src_scene;
  char* src_argv[6] = {argv[0], argv[6], argv[7], argv[8], argv[9], argv[5]};
  if (int rc = dst_scene.replay(6, argv, 6, "dst.raw dst_poses.bin dst_res dst_dim mu")) return rc;
  if (int rc = src_scene.replay(6, src_argv, 6, "src.raw src_poses.bin src_res src_dim mu")) return rc;
  DenseSLAMSystem& dst = *dst_scene.pipeline;
  DenseSLAMSystem& src = *src_scene.pipeline;
  const int dst_res = std::atoi(argv[3]), src_res = std::atoi(argv[8]);
  const float dst_dim = (float)std::atof(argv[4]);
  const double voxel = (double)dst_dim / dst_res;
  const double c30 = std::cos(M_PI / 6), s30 = std::sin(M_PI / 6);
  const double yaw[3][3] = {{c30, 0, s30}, {0, 1, 0}, {-s30, 0, c30}}, quarter[3][3] = {{0, -1, 0}, {1, 0, 0}, {0, 0, 1}};
  const double yaw_t[3] = {10.25, -3.5, 6.125}, quarter_t[3] = {2, -3, 4};
  struct Case { Eigen::Matrix4f T; int mode; float max_weight; };
  const Case cases[2] = {{about_centres(yaw, src_res, dst_res, voxel, yaw_t, false), SE_HIP_MERGE_FUSE, 100.f},
                         {about_centres(quarter, src_res, dst_res, voxel, quarter_t, true), SE_HIP_MERGE_FILL, 7.f}};
  long bad = 0;
  long long sum[4] = {0, 0, 0, 0};
  size_t blocks = 0;
  const Eigen::Matrix4f dst_pose = dst.getPose(), src_pose = src.getPose();
  for (const Case& c : cases) {
    std::shared_ptr<Map> before, source, after, source_after;
    dst.getMap(before);
    src.getMap(source);
    int64_t dev[10], host[10];
    for (int k = 0; k < 10; ++k) dev[k] = -7;
    const se_hip_merge_rule rule{c.mode, c.max_weight};
    float pull[12];
    if (!DenseSLAMSystem::rigidPull(c.T, dst_dim, dst_res, pull)) { std::fprintf(stderr, "rigidPull failed\n"); return 4; }
    if (!dst.mergeMapRigid(src, c.T, rule, dev)) { std::fprintf(stderr, "mergeMapRigid failed\n"); return 4; }
    se::merge_rule hr; hr.mode = c.mode; hr.max_weight = c.max_weight;
    se::merge_map_rigid(*before, *source, pull, hr, host);
    dst.getMap(after);
    src.getMap(source_after);
    const long d = differing(*before, *after) + differing(*source, *source_after);
    if (d != 0) { std::fprintf(stderr, "rigid merge mode %d: %ld octants / values / flags differ from the host's\n", c.mode, d); bad += d; }
    for (int k = 0; k < 10; ++k)
      if (dev[k] != host[k]) { std::fprintf(stderr, "counts[%d] device %lld host %lld\n", k, (long long)dev[k], (long long)host[k]); ++bad; }
    for (int k = 0; k < 4; ++k) sum[k] += dev[k];
    blocks = after->getBlockBuffer().size();
  }
  // a merge the library refuses (into itself; a transform with a scale) reports failure, and no merge moves a pose
  if (dst.mergeMapRigid(dst, cases[0].T)) ++bad;
  Eigen::Matrix4f scaled = cases[0].T;
  for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) scaled(r, c) *= 1.1f;
  if (dst.mergeMapRigid(src, scaled)) ++bad;
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) if (dst.getPose()(r, c) != dst_pose(r, c) || src.getPose()(r, c) != src_pose(r, c)) ++bad;
  std::printf("merges 2 combined %lld created %lld observed %lld both %lld blocks %zu bad %ld\n", sum[0], sum[1], sum[2], sum[3], blocks, bad);
  return 0;
}
