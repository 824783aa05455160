// DenseSLAMSystem::editMap (se_hip_edit_boxes_host) on a live handle against se::apply_edits (include/se/axis_aligned.hpp) applied to the
// getMap() snapshot taken before: SE_HIP_EDIT_STRICT, then SE_HIP_EDIT_REFERENCE on top of it, each compared voxel by voxel and node value by
// node value through a second getMap(), counts included.  Drives the mirror over a SLAMBench .raw stream with ground-truth poses, the way
// examples/denseslam_raw.cpp does.
//   usage: edit_mirror <scene.raw> <poses.bin> <volume_res> <volume_dim> <mu>
// Prints one line: "edits <n> voxels <n> nodes <n> blocks <n> invalid <n> changed <n> bad <n>" (the four counts summed over both modes;
// changed = voxels and node values whose bits differ from the first snapshot; bad = values or counts that differ from the host's).
#include "mirror_scene.hpp"
#include <se/axis_aligned.hpp>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <type_traits>
#include <vector>

typedef se::Octree<FieldType> Map;

// values whose bits differ between two snapshots of the same octants (-1: the octant sets differ)
static long differing(Map& a, Map& b) {
  if (a.getBlockBuffer().size() != b.getBlockBuffer().size() || a.getNodesBuffer().size() != b.getNodesBuffer().size()) return -1;
  long d = 0;
  for (size_t i = 0; i < a.getBlockBuffer().size(); ++i) {
    if (a.getBlockBuffer()[i]->code_ != b.getBlockBuffer()[i]->code_ || a.getBlockBuffer()[i]->active_ != b.getBlockBuffer()[i]->active_) return -1;
    for (int v = 0; v < 512; ++v) {
      const auto p = a.getBlockBuffer()[i]->voxel_block_[v], q = b.getBlockBuffer()[i]->voxel_block_[v];
      if (std::memcmp(&p.x, &q.x, sizeof p.x) || std::memcmp(&p.y, &q.y, sizeof p.y)) ++d;
    }
  }
  for (size_t i = 0; i < a.getNodesBuffer().size(); ++i) {
    if (a.getNodesBuffer()[i]->code_ != b.getNodesBuffer()[i]->code_) return -1;
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
  std::shared_ptr<Map> first;
  pipeline.getMap(first);
  if (first->getBlockBuffer().empty()) { std::fprintf(stderr, "empty map\n"); return 3; }
  const bool ofusion = std::is_same<FieldType, OFusion>::value;
  const se_hip_collide_test test = {0.f, ofusion ? 1 : 0};
  std::mt19937 rng(29);
  const auto& blocks = first->getBlockBuffer();
  long total[4] = {0, 0, 0, 0}, bad = 0, changed = 0;
  size_t n_edits = 0;
  for (int mode = SE_HIP_EDIT_STRICT; mode <= SE_HIP_EDIT_REFERENCE; ++mode) {
    // boxes: around allocated blocks, uniform, node octants, the whole volume, a few invalid ones
    std::vector<se_hip_edit> edits;
    auto add = [&](int x, int y, int z, int a, int b, int c) {
      se_hip_edit e;
      e.lo[0] = x; e.lo[1] = y; e.lo[2] = z; e.hi[0] = x + a; e.hi[1] = y + b; e.hi[2] = z + c;
      e.x = ofusion ? (float)((int)(rng() % 9) - 4) : (float)((int)(rng() % 9) - 4) * 0.25f;
      e.y = ofusion ? (float)(rng() % 8) * 0.5f : (float)(rng() % 101);
      e.flags = (uint32_t)(edits.size() % 16);
      e.only = (rng() % 3) ? 7u : 1u + (uint32_t)(rng() % 7);
      edits.push_back(e);
    };
    add(0, 0, 0, res, res, res);
    edits.back().flags = 15u; edits.back().only = 2u;   // "what is unseen becomes ..."
    for (int i = 0; i < 150; ++i) {
      const int* c = blocks[rng() % blocks.size()]->coordinates();
      add(c[0] + (int)(rng() % 20) - 10, c[1] + (int)(rng() % 20) - 10, c[2] + (int)(rng() % 20) - 10, 1 + (int)(rng() % 30), 1 + (int)(rng() % 30), 1 + (int)(rng() % 30));
    }
    for (int i = 0; i < 60; ++i) add((int)(rng() % (unsigned)(res + 32)) - 16, (int)(rng() % (unsigned)(res + 32)) - 16, (int)(rng() % (unsigned)(res + 32)) - 16, 1 + (int)(rng() % 64), 1 + (int)(rng() % 64), 1 + (int)(rng() % 64));
    for (int i = 0; i < 12; ++i) {
      const int s = 16 << (i % 3);
      const int* c = blocks[rng() % blocks.size()]->coordinates();
      add(c[0] / s * s, c[1] / s * s, c[2] / s * s, s, s, s);
      edits.back().flags = SE_HIP_EDIT_NODES | SE_HIP_EDIT_SET_X;
      edits.back().only = 7u;
    }
    add(5, 5, 5, 0, 9, 9); add(40, 40, 40, -9, 9, 9);
    add(0, 0, 0, 8, 8, 8); edits.back().lo[1] = -(1 << 30) - 1;
    add(0, 0, 0, 8, 8, 8); edits.back().flags = 32u;
    add(0, 0, 0, 8, 8, 8); edits.back().only = 0u;
    add(0, 0, 0, 8, 8, 8); edits.back().flags = 15u; edits.back().x = std::numeric_limits<float>::infinity();
    add(0, 0, 0, res, res, res); edits.back().flags = 15u; edits.back().only = 7u; edits.back().y = 100.5f;   // invalid for SDF only
    n_edits += edits.size();
    std::shared_ptr<Map> before, after;
    pipeline.getMap(before);
    int64_t dev[4] = {-1, -1, -1, -1}, host[4];
    if (!pipeline.editMap(edits.data(), edits.size(), &test, mode, dev)) { std::fprintf(stderr, "editMap failed\n"); return 4; }
    se::apply_edits(*before, edits.data(), edits.size(), &test, mode, host);
    pipeline.getMap(after);
    const long d = differing(*before, *after);
    if (d != 0) { std::fprintf(stderr, "mode %d: %ld values differ from the host's\n", mode, d); bad += d < 0 ? 1 : d; }
    for (int k = 0; k < 4; ++k) {
      if (dev[k] != host[k]) { std::fprintf(stderr, "mode %d: counts[%d] device %lld host %lld\n", mode, k, (long long)dev[k], (long long)host[k]); ++bad; }
      total[k] += (long)host[k];
    }
  }
  std::shared_ptr<Map> last;
  pipeline.getMap(last);
  changed = differing(*first, *last);
  std::printf("edits %zu voxels %ld nodes %ld blocks %ld invalid %ld changed %ld bad %ld\n", n_edits, total[0], total[1], total[2], total[3], changed, bad);
  return 0;
}
