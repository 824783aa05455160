// DenseSLAMSystem::allocateRegion (se_hip_allocate_boxes_host) on a live handle against se::allocate_boxes (include/se/allocate_region.hpp) applied
// to the getMap() snapshot taken before: a list of leaf and coarse boxes around and away from the fused surface, overlapping, clipped, empty and
// invalid ones, compared octant by octant, value by value and flag by flag through a second getMap(), counts included; then the same list again
// (nothing is created).  Drives the mirror over a SLAMBench .raw stream with ground-truth poses, the way examples/denseslam_raw.cpp does.
//   usage: alloc_mirror <scene.raw> <poses.bin> <volume_res> <volume_dim> <mu>
// Prints one line: "boxes <n> blocks <n> nodes <n> pairs <n> invalid <n> keys <n> again <n> bad <n>" (blocks / nodes created, requested pairs,
// invalid boxes, keys reported, octants the second call created; bad = octants, values, flags or counts that differ from the host's).
#include "mirror_scene.hpp"
#include <se/allocate_region.hpp>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <set>
#include <vector>

typedef se::Octree<FieldType> Map;

// octants, values or flags that differ between two snapshots
static long differing(Map& a, Map& b) {
  if (a.getBlockBuffer().size() != b.getBlockBuffer().size() || a.getNodesBuffer().size() != b.getNodesBuffer().size()) return 1;
  long d = 0;
  for (size_t i = 0; i < a.getBlockBuffer().size(); ++i) {
    if (a.getBlockBuffer()[i]->code_ != b.getBlockBuffer()[i]->code_ || a.getBlockBuffer()[i]->active_ != b.getBlockBuffer()[i]->active_) { ++d; continue; }
    for (int v = 0; v < 512; ++v) {
      const auto p = a.getBlockBuffer()[i]->voxel_block_[v], q = b.getBlockBuffer()[i]->voxel_block_[v];
      if (std::memcmp(&p.x, &q.x, sizeof p.x) || std::memcmp(&p.y, &q.y, sizeof p.y)) ++d;
    }
  }
  for (size_t i = 0; i < a.getNodesBuffer().size(); ++i) {
    if (a.getNodesBuffer()[i]->code_ != b.getNodesBuffer()[i]->code_ || a.getNodesBuffer()[i]->side_ != b.getNodesBuffer()[i]->side_) { ++d; continue; }
    for (int v = 0; v < 8; ++v) {
      const auto p = a.getNodesBuffer()[i]->value_[v], q = b.getNodesBuffer()[i]->value_[v];
      if (std::memcmp(&p.x, &q.x, sizeof p.x) || std::memcmp(&p.y, &q.y, sizeof p.y)) ++d;
    }
  }
  return d;
}

int main(int argc, char** argv) {
  MirrorScene scene;
  if (int rc = scene.replay(argc, argv, 6, "scene.raw poses.bin res dim mu")) return rc;
  DenseSLAMSystem& pipeline = *scene.pipeline;
  const int res = scene.res;
  std::shared_ptr<Map> before, after, last;
  pipeline.getMap(before);
  if (before->getBlockBuffer().empty()) { std::fprintf(stderr, "empty map\n"); return 3; }
  int leaf = -3;
  for (int s = res; s > 1; s >>= 1) ++leaf;
  std::mt19937 rng(31);
  std::vector<se_hip_alloc_box> boxes;
  auto add = [&](int x, int y, int z, int a, int b, int c, int level) {
    se_hip_alloc_box r;
    r.lo[0] = x; r.lo[1] = y; r.lo[2] = z; r.hi[0] = x + a; r.hi[1] = y + b; r.hi[2] = z + c; r.level = level; r.reserved = 0;
    boxes.push_back(r);
  };
  const auto& blocks = before->getBlockBuffer();
  for (int i = 0; i < 60; ++i) {   // around the fused surface: partly existing, partly new
    const int* c = blocks[rng() % blocks.size()]->coordinates();
    add(c[0] + (int)(rng() % 40) - 20, c[1] + (int)(rng() % 40) - 20, c[2] + (int)(rng() % 40) - 20, 1 + (int)(rng() % 30), 1 + (int)(rng() % 30), 1 + (int)(rng() % 30), 0);
  }
  for (int i = 0; i < 60; ++i)     // anywhere, any level, some partly or wholly outside
    add((int)(rng() % (unsigned)(res + 32)) - 16, (int)(rng() % (unsigned)(res + 32)) - 16, (int)(rng() % (unsigned)(res + 32)) - 16, 1 + (int)(rng() % 48), 1 + (int)(rng() % 48),
        1 + (int)(rng() % 48), (int)(rng() % (unsigned)(leaf + 1)));
  add(0, 0, 0, 8, 8, 8, 0); add(0, 0, 0, 64, 64, 64, 0); add(16, 16, 16, 40, 40, 40, 0);   // the origin block; overlapping
  add(res - 5, res - 5, res - 5, 30, 30, 30, 0); add(-20, 8, 8, 24, 4, 4, 2);                 // clipped
  add(5, 5, 5, 0, 9, 9, 0); add(40, 40, 40, -9, 9, 9, 1);                                     // empty, inverted
  add(0, 0, 0, 8, 8, 8, 0); boxes.back().lo[1] = -(1 << 30) - 1;
  add(0, 0, 0, 8, 8, 8, leaf + 1);
  add(0, 0, 0, 8, 8, 8, -1);
  add(0, 0, 0, 8, 8, 8, 0); boxes.back().reserved = 7u;
  long bad = 0;
  int64_t dev[4] = {-1, -1, -1, -1}, host[4], again[4] = {-1, -1, -1, -1};
  std::vector<uint64_t> keys((size_t)1 << 20);
  if (!pipeline.allocateRegion(boxes.data(), boxes.size(), dev, keys.data(), (int64_t)keys.size())) { std::fprintf(stderr, "allocateRegion failed\n"); return 4; }
  std::vector<se::key_t> host_keys;
  std::set<uint64_t> had;
  for (auto& p : before->getNodesBuffer()) had.insert(p->code_);
  for (auto& p : before->getBlockBuffer()) had.insert(p->code_);
  se::allocate_boxes(*before, boxes.data(), boxes.size(), host, &host_keys);
  pipeline.getMap(after);
  const long d = differing(*before, *after);
  if (d != 0) { std::fprintf(stderr, "%ld octants / values / flags differ from the host's\n", d); bad += d; }
  for (int k = 0; k < 4; ++k)
    if (dev[k] != host[k]) { std::fprintf(stderr, "counts[%d] device %lld host %lld\n", k, (long long)dev[k], (long long)host[k]); ++bad; }
  // the device's keys: none twice, none of an octant that existed, and with the map before they imply the map after
  const uint64_t nk = keys[0];
  if (nk + 1 > keys.size()) { std::fprintf(stderr, "key list too small\n"); return 5; }
  std::set<uint64_t> implied = had, got;
  for (uint64_t i = 0; i < nk; ++i) {
    const uint64_t k = keys[1 + i];
    if (had.count(k)) ++bad;
    const int level = (int)(k & 0x1FF);
    for (int l = level; l >= 1; --l) implied.insert(((k & ~0x1FFull) & ~((1ull << (3 * (leaf + 3 - l))) - 1ull)) | (uint64_t)l);
  }
  if (std::set<uint64_t>(keys.begin() + 1, keys.begin() + 1 + nk).size() != nk) ++bad;
  for (auto& p : after->getNodesBuffer()) got.insert(p->code_);
  for (auto& p : after->getBlockBuffer()) got.insert(p->code_);
  if (implied != got) { std::fprintf(stderr, "the keys do not imply the map\n"); ++bad; }
  if (!pipeline.allocateRegion(boxes.data(), boxes.size(), again)) return 4;
  pipeline.getMap(last);
  if (differing(*after, *last) != 0 || again[2] != dev[2] || again[3] != dev[3]) ++bad;
  std::printf("boxes %zu blocks %lld nodes %lld pairs %lld invalid %lld keys %llu again %lld bad %ld\n", boxes.size(), (long long)dev[0], (long long)dev[1],
              (long long)dev[2], (long long)dev[3], (unsigned long long)nk, (long long)(again[0] + again[1]), bad);
  return 0;
}
