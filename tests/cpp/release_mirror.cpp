// DenseSLAMSystem::releaseMap (se_hip_release_boxes) on a live handle against se::release_map (include/se/release_map.hpp) applied to the getMap()
// snapshot taken before: no records, the octants that hold nothing anywhere, a list of 70 mixed records, the centre box forgotten, the whole volume
// forgotten -- one after the other, each compared octant by octant, value by value and flag by flag through a second getMap(), counts and touched
// box included; the poses stay where they are; a record the library refuses changes nothing.
// Drives the mirror over a SLAMBench .raw stream with ground-truth poses, the way examples/denseslam_raw.cpp does.
//   usage: release_mirror <scene.raw> <poses.bin> <volume_res> <volume_dim> <mu>
// Prints one line: "calls <n> kept <n> released <n> nodes_kept <n> nodes_released <n> observed <n> unseen_only <n> left <n> bad <n>" (the counts
// summed over the calls; unseen_only = blocks the second call released; left = blocks after the last one; bad = octants, values, flags, counts,
// box or pose components that differ from the host's).
#include "mirror_scene.hpp"
#include <se/release_map.hpp>

#include <cstdio>
#include <cstring>
#include <vector>

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

static se_hip_release_box box(int x, int y, int z, int sx, int sy, int sz, int what) {
  se_hip_release_box b;
  b.lo[0] = x; b.lo[1] = y; b.lo[2] = z; b.side[0] = sx; b.side[1] = sy; b.side[2] = sz; b.what = what; b.reserved = 0;
  return b;
}

int main(int argc, char** argv) {
  MirrorScene scene;
  if (int rc = scene.replay(argc, argv, 6, "scene.raw poses.bin res dim mu")) return rc;
  DenseSLAMSystem& pipeline = *scene.pipeline;
  const int res = scene.res, q = res / 4;
  std::vector<std::vector<se_hip_release_box>> calls(5);
  calls[1].push_back(box(0, 0, 0, res, res, res, SE_HIP_RELEASE_UNSEEN));
  // 70 records, so that a wave's record loop takes two steps: slabs of unequal thickness in both codes, boxes that cut blocks, duplicates
  unsigned long long seed = 12345;
  auto next = [&](int m) { seed = seed * 6364136223846793005ull + 1442695040888963407ull; return (int)((seed >> 33) % (unsigned)m); };
  for (int i = 0; i < 68; ++i)
    calls[2].push_back(box(next(res) - 8, next(res) - 8, next(res) - 8, 1 + next(res / 2), 1 + next(res / 2), 1 + next(res / 2), next(2) ? SE_HIP_RELEASE_ALL : SE_HIP_RELEASE_UNSEEN));
  calls[2].push_back(calls[2][3]);
  calls[2].push_back(box(q, q, q - 3, q, q, 2 * q + 3, SE_HIP_RELEASE_ALL));
  calls[3].push_back(box(q, q, q, 2 * q, 2 * q, 2 * q, SE_HIP_RELEASE_ALL));
  calls[4].push_back(box(-8, -8, -8, res + 16, res + 16, res + 16, SE_HIP_RELEASE_ALL));
  long bad = 0;
  long long sum[5] = {0, 0, 0, 0, 0}, unseen_only = 0;
  size_t left = 0;
  for (size_t c = 0; c < calls.size(); ++c) {
    std::shared_ptr<Map> before, after;
    pipeline.getMap(before);
    const Eigen::Matrix4f pose = pipeline.getPose();
    int64_t dev[5] = {-1, -1, -1, -1, -1}, host[5];
    int32_t dev_box[6] = {-1, -1, -1, -1, -1, -1}, host_box[6];
    if (!pipeline.releaseMap(calls[c], dev, dev_box)) { std::fprintf(stderr, "releaseMap failed\n"); return 4; }
    if (!se::release_map(*before, calls[c].data(), calls[c].size(), host, host_box)) { std::fprintf(stderr, "release_map refused call %zu\n", c); return 4; }
    pipeline.getMap(after);
    const long d = differing(*before, *after);
    if (d != 0) { std::fprintf(stderr, "call %zu: %ld octants / values / flags differ from the host's\n", c, d); bad += d; }
    for (int k = 0; k < 5; ++k) {
      if (dev[k] != host[k]) { std::fprintf(stderr, "call %zu counts[%d] device %lld host %lld\n", c, k, (long long)dev[k], (long long)host[k]); ++bad; }
      sum[k] += dev[k];
    }
    for (int k = 0; k < 6; ++k)
      if (dev_box[k] != host_box[k]) { std::fprintf(stderr, "call %zu touched[%d] device %d host %d\n", c, k, dev_box[k], host_box[k]); ++bad; }
    if (c == 1) unseen_only = dev[1];
    for (int r = 0; r < 4; ++r)
      for (int k = 0; k < 4; ++k) if (pipeline.getPose()(r, k) != pose(r, k)) ++bad;
    left = after->getBlockBuffer().size();
  }
  // a record the library refuses changes nothing
  std::vector<se_hip_release_box> wrong(1, box(0, 0, 0, res, 0, res, SE_HIP_RELEASE_ALL));
  if (pipeline.releaseMap(wrong)) ++bad;
  std::printf("calls %zu kept %lld released %lld nodes_kept %lld nodes_released %lld observed %lld unseen_only %lld left %zu bad %ld\n", calls.size(), sum[0], sum[1],
              sum[2], sum[3], sum[4], unseen_only, left, bad);
  return 0;
}
