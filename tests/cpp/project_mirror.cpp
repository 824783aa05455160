// DenseSLAMSystem::projectColumns (se_hip_project_columns_host) on a replayed scene: per axis and stop_at one request over the whole footprint
// grown by 8 voxels on every side, five layers (the full height, the height grown by 9, a 16-voxel band, a one-voxel slice and
// [-2^20, 2^20)).  The four arrays are hashed for the comparison with the Python entry on the same frames, and held cell for cell to
// se::geometry::project_columns (include/se/project_columns.hpp) on the getMap() snapshot.
//   usage: project_mirror <scene.raw> <poses.bin> <volume_res> <volume_dim> <mu>
// Prints one line of `key value` pairs: "cells <n>" per request, "hash_<axis>_<stop_at> <h>" per request with
// h = sum over the arrays status, first, last, count (in this order, indices running on) of (uint32(value) + 1) * ((index + 1) * G) mod 2^64,
// G = 0x9E3779B97F4A7C15, then "occupied <n> none <n>" (cells with status occupied / without a blocking voxel, over all requests) and
// "bad <n>" (cells that differ from the host restatement).
#include "mirror_scene.hpp"
#include <se/project_columns.hpp>

#include <cstdio>
#include <cstring>
#include <type_traits>
#include <vector>

int main(int argc, char** argv) {
  MirrorScene scene;
  if (int rc = scene.replay(argc, argv, 6, "scene.raw poses.bin res dim mu")) return rc;
  DenseSLAMSystem& pipeline = *scene.pipeline;
  const int res = scene.res;
  std::shared_ptr<se::Octree<FieldType> > map;
  pipeline.getMap(map);
  if (map->getBlockBuffer().empty()) { std::fprintf(stderr, "empty map\n"); return 3; }

  const bool ofusion = std::is_same<FieldType, OFusion>::value;
  const se_hip_collide_test test = {0.f, ofusion ? 1 : 0};
  const se::geometry::voxel_test<FieldType> host_test = {0.f, ofusion};
  const int layers[5][2] = {{0, res}, {-9, res + 9}, {res / 4, res / 4 + 16}, {res / 2, res / 2 + 1}, {-(1 << 20), 1 << 20}};
  long occupied = 0, none = 0, bad = 0;
  size_t cells = 0;
  std::vector<unsigned long long> hashes;
  for (int axis = 0; axis < 3; ++axis)
    for (int s = 0; s < 2; ++s) {
      se_hip_project_request rq;
      std::memset(&rq, 0, sizeof rq);
      rq.axis = axis;
      rq.lo[0] = rq.lo[1] = -8;
      rq.side[0] = rq.side[1] = res + 16;
      rq.n_layers = 5;
      for (int l = 0; l < 5; ++l) { rq.layers[l][0] = layers[l][0]; rq.layers[l][1] = layers[l][1]; }
      rq.stop_at = s ? SE_HIP_COLLISION_UNSEEN : SE_HIP_COLLISION_OCCUPIED;
      cells = (size_t)5 * rq.side[0] * rq.side[1];
      std::vector<uint8_t> status(cells), status_only(cells);
      std::vector<int32_t> first(cells), last(cells), count(cells);
      se_hip_project_out out = {status.data(), first.data(), last.data(), count.data()};
      if (!pipeline.projectColumns(rq, test, out)) { std::fprintf(stderr, "projectColumns failed\n"); return 4; }
      se_hip_project_out out1 = {status_only.data(), nullptr, nullptr, nullptr};
      if (!pipeline.projectColumns(rq, test, out1)) { std::fprintf(stderr, "projectColumns failed\n"); return 4; }

      se::geometry::project_request hr;
      hr.axis = axis;
      for (int k = 0; k < 2; ++k) { hr.lo[k] = rq.lo[k]; hr.side[k] = rq.side[k]; }
      hr.n_layers = 5;
      for (int l = 0; l < 5; ++l) { hr.layers[l][0] = layers[l][0]; hr.layers[l][1] = layers[l][1]; }
      hr.stop_at = s ? se::geometry::collision_status::unseen : se::geometry::collision_status::occupied;
      const std::vector<se::geometry::project_cell> host = se::geometry::project_columns(*map, hr, host_test);
      unsigned long long h = 0, index = 0;
      const unsigned long long G = 0x9E3779B97F4A7C15ull;
      for (size_t i = 0; i < cells; ++i) h += ((unsigned long long)status[i] + 1ull) * (++index * G);
      for (size_t i = 0; i < cells; ++i) h += ((unsigned long long)(uint32_t)first[i] + 1ull) * (++index * G);
      for (size_t i = 0; i < cells; ++i) h += ((unsigned long long)(uint32_t)last[i] + 1ull) * (++index * G);
      for (size_t i = 0; i < cells; ++i) h += ((unsigned long long)(uint32_t)count[i] + 1ull) * (++index * G);
      hashes.push_back(h);
      for (size_t i = 0; i < cells; ++i) {
        const bool same = (int)host[i].status == (int)status[i] && status_only[i] == status[i] && host[i].first == first[i] && host[i].last == last[i] &&
                          host[i].count == count[i];
        if (!same) {
          if (bad < 5)
            std::fprintf(stderr, "axis %d stop_at %d cell %zu: host %d %d %d %d, device %d %d %d %d (status alone %d)\n", axis, s, i, (int)host[i].status, host[i].first,
                         host[i].last, host[i].count, (int)status[i], (int)first[i], (int)last[i], (int)count[i], (int)status_only[i]);
          ++bad;
        }
        occupied += status[i] == SE_HIP_COLLISION_OCCUPIED;
        none += count[i] == 0;
      }
    }
  std::printf("cells %zu", cells);
  for (int axis = 0; axis < 3; ++axis)
    for (int s = 0; s < 2; ++s) std::printf(" hash_%d_%d %llu", axis, s, hashes[(size_t)axis * 2 + s]);
  std::printf(" occupied %ld none %ld bad %ld\n", occupied, none, bad);
  return 0;
}
