/*
 * DenseSLAMSystem -- C++ mirror of the reference's pipeline class for the hot path
 *   se_denseslam/include/se/DenseSLAMSystem.h:58-411  (class DenseSLAMSystem)
 * on top of the C ABI of include/se_hip.h.  Header-only: an application written against the
 * reference class includes this header instead, defines SE_FIELD_TYPE (SDF or OFusion, as the
 * reference requires: DenseSLAMSystem.h:54) and links libse_hip.so.
 *
 * What is kept (same names, argument meaning and "did the stage run" return values):
 *   the two constructors, preprocessing() (mm -> metres, preprocessing.cpp:161-188, fused into the
 *   upload; the optional bilateral filter runs on the device in front of tracking()), integration(),
 *   tracking(), raycasting(), setPose()/getPose()/getPosition()/getInitPos(), getIntegrated(), getTracked(),
 *   getModelDimensions()/getModelResolution()/getComputationResolution(), renderVolume()/renderTrack()/
 *   renderDepth(), dump_mesh(), setViewPose()/getViewPose(), synchroniseDevices().
 * What differs, because the map lives in HBM:
 *   getMap(std::shared_ptr<se::Octree<FieldType>>&) materialises the device map as a host pointer octree with the reference's
 *   node / block layout and read interface (include/se/octree.hpp) -- a snapshot, not the live map; getMap(MapSnapshot&) is
 *   the flat form (blocks sorted by Morton key); getVertexNormal() downloads vertex_/normal_.
 *   tracking() runs the reference's ICP on the device; poses can still be injected
 *   with setPose(), as the reference's GUI does with ground truth (se_apps/src/mainQt.cpp:257-265).
 *   renderVolume / renderTrack / renderDepth shade on the device and copy the RGBW image out.
 * Errors of the C ABI are reported like the reference reports its own failures: message on
 * std::cerr; constructors additionally throw std::runtime_error (the reference would dereference
 * an unallocated map).
 */
#ifndef SE_HIP_DENSESLAMSYSTEM_H
#define SE_HIP_DENSESLAMSYSTEM_H

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <iostream>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "../se_hip.h"

#include "config.h"       /* the reference's Configuration, field for field (+ hip_device, hip_max_blocks) */
#include "eigen_pods.h"
#include "octree.hpp"     /* SDF / OFusion field types, se::Octree<FieldType> host mirror for getMap() */

#ifndef SE_FIELD_TYPE
#error "define SE_FIELD_TYPE to SDF or OFusion before including se/DenseSLAMSystem.h (as the reference requires)"
#endif
typedef SE_FIELD_TYPE FieldType;

struct MapSnapshot {
  int n_blocks = 0, n_nodes = 0;
  std::vector<int32_t> coords;   /* [n][3] block min corners (voxels), sorted by Morton key */
  std::vector<float> x, y;       /* [n][512], voxel index x + 8y + 64z */
  std::vector<uint8_t> active;
};

class DenseSLAMSystem {
 public:
  DenseSLAMSystem(const Eigen::Vector2i& inputSize, const Eigen::Vector3i& volumeResolution,
                  const Eigen::Vector3f& volumeDimensions, const Eigen::Vector3f& initPose, std::vector<int>& pyramid,
                  const Configuration& config)
      : DenseSLAMSystem(inputSize, volumeResolution, volumeDimensions, toMatrix4f(initPose), pyramid, config) {}

  DenseSLAMSystem(const Eigen::Vector2i& inputSize, const Eigen::Vector3i& volumeResolution,
                  const Eigen::Vector3f& volumeDimensions, const Eigen::Matrix4f& initPose, std::vector<int>& pyramid,
                  const Configuration& config)
      : computation_size_(inputSize), volume_resolution_(volumeResolution), volume_dimension_(volumeDimensions) {
    iterations_.assign(pyramid.begin(), pyramid.end());
    if (iterations_.empty()) iterations_ = {10, 5, 4};
    init_pose_ = Eigen::Vector3f(initPose(0, 3), initPose(1, 3), initPose(2, 3));
    mu_ = config.mu;
    pose_ = initPose;
    raycast_pose_ = initPose;
    se_hip_config c{};
    c.width = inputSize.x(); c.height = inputSize.y();
    c.volume_resolution = volumeResolution.x(); c.volume_dimension = volumeDimensions.x();
    c.field_type = is_sdf() ? SE_HIP_FIELD_SDF : SE_HIP_FIELD_OFUSION;
    c.device = config.hip_device; c.max_blocks = config.hip_max_blocks;
    if (se_hip_create(&c, &h_) != SE_HIP_OK) throw std::runtime_error(std::string("DenseSLAMSystem: ") + se_hip_last_error());
    /* The class never hands out device pointers: every way an application can look at vertex_ / normal_ (tracking, render*, getVertexNormal)
     * is an API call that launches a held-back raycast first, so the one-queue streaming schedule is safe by construction here. */
    if (config.hip_streaming) se_hip_set_streaming(h_, 1);
    if (config.hip_pinned_input) se_hip_set_pinned_input(h_, 1);
    live().push_back(h_);
  }
  ~DenseSLAMSystem() {
    std::vector<se_hip_pipeline*>& l = live();
    l.erase(std::remove(l.begin(), l.end(), h_), l.end());
    se_hip_destroy(h_);
  }
  DenseSLAMSystem(const DenseSLAMSystem&) = delete;
  DenseSLAMSystem& operator=(const DenseSLAMSystem&) = delete;

  /* DenseSLAMSystem.h:147 / DenseSLAMSystem.cpp:128-141 */
  bool preprocessing(const unsigned short* inputDepth, const Eigen::Vector2i& inputSize, const bool filterInput) {
    // bilateralFilterKernel feeds only the tracking pyramid (scaled_depth_[0]); it runs inside se_hip_track
    return ok(se_hip_filter_depth(h_, filterInput ? 1 : 0)) && ok(se_hip_upload_depth_mm(h_, inputDepth, inputSize.x(), inputSize.y()));
  }
  /* DenseSLAMSystem.h:154-157: declared with "TODO Implement this." in the reference and never defined; the RGB image has no
   * consumer in the pipeline (se-denseslam is depth-only), so the overload forwards to the depth-only form. */
  bool preprocessing(const unsigned short* inputDepth, const unsigned char* /*inputRGB*/, const Eigen::Vector2i& inputSize, const bool filterInput) {
    return preprocessing(inputDepth, inputSize, filterInput);
  }
  /* the reference's float_depth_ handed over directly (metres) */
  bool preprocessing(const float* depthMetres) { return ok(se_hip_upload_depth(h_, depthMetres)); }
  /* page-locked host memory for a frame reader's input buffer (Configuration::hip_pinned_input: such images are not copied by preprocessing()) */
  static void* allocateInput(size_t bytes) { return se_hip_host_alloc(bytes); }
  static void freeInput(void* host) { se_hip_host_free(host); }
  /* ... or left where a device-side producer put it (HBM, metres, valid until the next call): no copy at all */
  bool preprocessingDevice(const float* deviceDepthMetres) { return ok(se_hip_set_depth_device(h_, deviceDepthMetres)); }

  /* DenseSLAMSystem.h:173 / DenseSLAMSystem.cpp:143-189: ICP against the last raycast, on the device */
  bool tracking(const Eigen::Vector4f& k, float icp_threshold, unsigned tracking_rate, unsigned frame) {
    const int r = se_hip_track(h_, k.data(), icp_threshold, tracking_rate, frame, iterations_.data(), (int32_t)iterations_.size(), pose_.data());
    ok(r);
    tracked_ = r > 0;
    return tracked_;
  }

  /* DenseSLAMSystem.h:193 / DenseSLAMSystem.cpp:206-268 */
  bool integration(const Eigen::Vector4f& k, unsigned int integration_rate, float mu, unsigned int frame) {
    const int r = se_hip_integrate(h_, pose_.data(), k.data(), integration_rate, mu, frame);
    ok(r);
    integrated_ = r > 0;
    return r > 0;
  }
  /* DenseSLAMSystem.h:212 / DenseSLAMSystem.cpp:191-204 */
  bool raycasting(const Eigen::Vector4f& k, float mu, unsigned int frame) {
    /* held back until the next integration()'s allocation scan (one launch for both) on a streaming handle, se_hip_raycast otherwise */
    const int r = se_hip_raycast_deferred(h_, pose_.data(), k.data(), mu, frame);
    ok(r);
    if (r > 0) raycast_pose_ = pose_;
    return r > 0;
  }

  /* DenseSLAMSystem.h:241-286 / DenseSLAMSystem.cpp:274-300: RGBW images of the computation size */
  void renderVolume(unsigned char* out, const Eigen::Vector2i& outputSize, int frame, int raycast_rendering_rate,
                    const Eigen::Vector4f& k, float largestep) {
    (void)outputSize;
    ok(se_hip_render_volume(h_, out, viewPose_->data(), k.data(), mu_, largestep, (uint32_t)frame, (uint32_t)raycast_rendering_rate));
  }
  void renderTrack(unsigned char* out, const Eigen::Vector2i& outputSize) { (void)outputSize; ok(se_hip_render_track(h_, out)); }
  void renderDepth(unsigned char* out, const Eigen::Vector2i& outputSize) { (void)outputSize; ok(se_hip_render_depth(h_, out)); }

  /* DenseSLAMSystem.h:224 / DenseSLAMSystem.cpp:302-322: marching cubes of the map into a VTK file */
  void dump_mesh(const std::string filename) { ok(se_hip_dump_mesh(h_, filename.c_str())); }
  /* DenseSLAMSystem.h:219: declared, called by se_apps/src/benchmark.cpp:187, and EMPTY in the reference
   * (DenseSLAMSystem.cpp:270-272) -- kept empty so that an application behaves the same; saveMap() is the useful thing */
  void dump_volume(const std::string) {}
  /* the whole map in Octree::save's byte layout, and back (Octree::load without its defects, see se_hip.h) */
  bool saveMap(const std::string& filename) { return ok(se_hip_save_map(h_, filename.c_str())); }
  bool loadMap(const std::string& filename) { return ok(se_hip_load_map(h_, filename.c_str())); }
  void setViewPose(Eigen::Matrix4f* value = NULL) { viewPose_ = value ? value : &pose_; }   /* DenseSLAMSystem.h:363-372 */
  Eigen::Matrix4f* getViewPose() { return viewPose_; }

  /* DenseSLAMSystem.h:295: the reference shares its live se::Octree; here the device map is materialised as a host
   * se::Octree<FieldType> (include/se/octree.hpp) with the reference's node / block member layout and read interface */
  void getMap(std::shared_ptr<se::Octree<FieldType> >& out) {
    out = std::make_shared<se::Octree<FieldType> >();
    out->init(volume_resolution_.x(), volume_dimension_.x());
    int nb = 0, nn = 0;
    if (!ok(se_hip_counts(h_, &nb, &nn))) return;
    std::vector<uint64_t> code(nn);
    std::vector<uint32_t> side(nn);
    std::vector<float> nx((size_t)nn * 8), ny((size_t)nn * 8);
    if (!ok(se_hip_download_nodes(h_, code.data(), side.data(), nx.data(), ny.data()))) return;
    for (int i = 0; i < nn; ++i) {
      se::Node<FieldType>* n = out->add_node(code[i], side[i]);
      for (int j = 0; j < 8; ++j) { n->value_[j].x = nx[(size_t)i * 8 + j]; n->value_[j].y = ny[(size_t)i * 8 + j]; }
    }
    MapSnapshot snap;
    getMap(snap);
    int max_level = 0;
    for (int s = volume_resolution_.x(); s > 1; s >>= 1) ++max_level;
    for (int i = 0; i < snap.n_blocks; ++i) {
      const int* c = &snap.coords[(size_t)i * 3];
      uint64_t key = 0;
      for (int b = 0; b < max_level; ++b)
        key |= ((uint64_t)((c[0] >> b) & 1) << (3 * b)) | ((uint64_t)((c[1] >> b) & 1) << (3 * b + 1)) | ((uint64_t)((c[2] >> b) & 1) << (3 * b + 2));
      se::VoxelBlock<FieldType>* blk = out->add_block(key | (uint64_t)(max_level - 3), c, snap.active[i] != 0);
      for (int v = 0; v < 512; ++v) { blk->voxel_block_[v].x = snap.x[(size_t)i * 512 + v]; blk->voxel_block_[v].y = snap.y[(size_t)i * 512 + v]; }
    }
    out->finalize();
  }
  void getMap(MapSnapshot& out) {
    int nb = 0, nn = 0;
    if (!ok(se_hip_counts(h_, &nb, &nn))) return;
    out.n_blocks = nb; out.n_nodes = nn;
    out.coords.resize((size_t)nb * 3); out.x.resize((size_t)nb * 512); out.y.resize((size_t)nb * 512); out.active.resize(nb);
    if (nb) ok(se_hip_download_blocks(h_, out.coords.data(), out.x.data(), out.y.data(), out.active.data()));
  }
  /* Not in the reference's class (an addition of this mirror): VolumeTemplate::get / operator[] / interp / grad for n points in metres
   * (host_points_m[n][3]) answered on the device map without getMap() -- se_hip_query_points_host, definitions in se_hip.h.  host_out
   * holds host arrays; a null member is not computed. */
  bool queryMap(const float* host_points_m, size_t n, se_hip_query_out& host_out) {
    return ok(se_hip_query_points_host(h_, host_points_m, (int64_t)n, &host_out));
  }
  /* Not in the reference's class (an addition of this mirror): se::geometry::collides_with for n axis-aligned boxes (host_boxes[n][6]: lo xyz,
   * side xyz in voxels) answered on the device map without getMap() -- se_hip_collide_boxes_host, definitions in se_hip.h.  mode
   * SE_HIP_COLLIDE_REFERENCE returns what collides_with (include/se/octree_collision.hpp) returns on the getMap() snapshot, SE_HIP_COLLIDE_STRICT
   * the min over the box's voxels; host_status[n] receives 0 occupied, 1 unseen, 2 empty, 255 invalid box. */
  bool collidesWith(const int32_t* host_boxes, size_t n, const se_hip_collide_test& test, int32_t mode, uint8_t* host_status) {
    return ok(se_hip_collide_boxes_host(h_, host_boxes, (int64_t)n, &test, mode, host_status));
  }
  /* Not in the reference's class: collision queries for n boxes moved along straight segments (host_motions[n][9]: lo xyz, side xyz, d xyz in
   * voxels), exact for the continuous motion -- se_hip_collide_motions_host, definitions in se_hip.h.  host_out.status is required; a null
   * host_out.t_first means "not wanted".  stop_at is SE_HIP_COLLISION_OCCUPIED or SE_HIP_COLLISION_UNSEEN.  The answers are those of
   * se::geometry::motion_status_and_entry (include/se/motion_collision.hpp) on the getMap() snapshot. */
  bool collidesMoving(const int32_t* host_motions, size_t n, const se_hip_collide_test& test, int32_t stop_at, se_hip_motion_out& host_out) {
    return ok(se_hip_collide_motions_host(h_, host_motions, (int64_t)n, &test, stop_at, &host_out));
  }
  /* Not in the reference's class: clearance queries for n boxes (host_queries[n][7]: lo xyz, side xyz, r_max in voxels) -- the squared
   * distance to the nearest blocking voxel within r_max and that voxel -- se_hip_clearance_boxes_host, definitions in se_hip.h.  host_out.d2 is
   * required; a null host_out.nearest means "not wanted".  stop_at is SE_HIP_COLLISION_OCCUPIED or SE_HIP_COLLISION_UNSEEN.  The answers are
   * those of se::geometry::clearance (include/se/clearance.hpp) on the getMap() snapshot. */
  bool clearanceOf(const int32_t* host_queries, size_t n, const se_hip_collide_test& test, int32_t stop_at, se_hip_clearance_out& host_out) {
    return ok(se_hip_clearance_boxes_host(h_, host_queries, (int64_t)n, &test, stop_at, &host_out));
  }
  /* Not in the reference's class: column projections of the map -- per cell of a 2D footprint and per interval along request.axis the min
   * class, the first and the last blocking voxel and the number of blocking voxels -- se_hip_project_columns_host, definitions in
   * se_hip.h.  The arrays of host_out are [n_layers][side[1]][side[0]]; host_out.status is required, a null first / last / count means "not
   * wanted".  The answers are those of se::geometry::project_columns (include/se/project_columns.hpp) on the getMap() snapshot. */
  bool projectColumns(const se_hip_project_request& request, const se_hip_collide_test& test, se_hip_project_out& host_out) {
    return ok(se_hip_project_columns_host(h_, &request, &test, &host_out));
  }
  /* Not in the reference's class: the distance field of a region -- for every voxel v of [lo, lo + side) what clearanceOf answers for the box
   * [v, v + robot) with request.r_max and request.stop_at -- se_hip_distance_field_host, definitions in se_hip.h.  The arrays of host_out are
   * [side z][side y][side x] (nearest: [3] more); host_out.d2 is required, a null host_out.nearest means "not wanted".  The answers are those
   * of se::geometry::distance_field (include/se/distance_field.hpp) on the getMap() snapshot. */
  bool distanceField(const se_hip_field_request& request, const se_hip_collide_test& test, se_hip_field_out& host_out) {
    return ok(se_hip_distance_field_host(h_, &request, &test, &host_out));
  }
  /* Not in the reference's class: the reachability field of a region -- for every position v of [lo, lo + side) the number of moves of the
   * box [v, v + robot) to the nearest usable seed through free positions of the region, that seed, and the first move of a shortest path
   * -- se_hip_reach_field_host, definitions in se_hip.h.  The arrays of host_out are [side z][side y][side x]; host_out.steps is required, a
   * null seed / next / counts means "not wanted"; request.seeds and host_out.counts are host pointers.  The answers are those of
   * se::geometry::reach_field (include/se/reach_field.hpp) on the getMap() snapshot. */
  bool reachField(const se_hip_reach_request& request, const se_hip_collide_test& test, se_hip_reach_out& host_out) {
    return ok(se_hip_reach_field_host(h_, &request, &test, &host_out));
  }
  /* Not in the reference's class: collision queries for n oriented boxes (host_boxes[n][12]: centre xyz, then the half-axes h0, h1, h2 xyz, in
   * sub-units of 1 / SE_HIP_ORIENTED_SUB voxel), exact for the box given -- se_hip_collide_oriented_host, definitions in se_hip.h.
   * host_status[n] receives 0 occupied, 1 unseen, 2 empty, 255 invalid box.  The answers are those of se::geometry::oriented_status
   * (include/se/oriented_collision.hpp) on the getMap() snapshot. */
  bool collidesOriented(const int32_t* host_boxes, size_t n, const se_hip_collide_test& test, uint8_t* host_status) {
    return ok(se_hip_collide_oriented_host(h_, host_boxes, (int64_t)n, &test, host_status));
  }
  /* The twelve int32 of one such box from a metric one: box_to_world holds the box's axes in the columns of its rotation and its centre in
   * its translation (metres), half_extents_m the half lengths along those axes.  The centre and the three scaled columns are rounded to the
   * nearest sub-unit; the query is exact for the rounded box, which lies within sqrt(3) / 8 voxel of the one asked for
   * (se::geometry::oriented_box_round of include/se/oriented_collision.hpp does the same on plain arrays). */
  void orientedBox(const Eigen::Matrix4f& box_to_world, const Eigen::Vector3f& half_extents_m, int32_t out[12]) const {
    const double scale = (double)SE_HIP_ORIENTED_SUB * volume_resolution_.x() / volume_dimension_.x();
    for (int k = 0; k < 3; ++k) out[k] = (int32_t)std::nearbyint(box_to_world(k, 3) * scale);
    for (int i = 0; i < 3; ++i)
      for (int k = 0; k < 3; ++k) out[3 + 3 * i + k] = (int32_t)std::nearbyint((double)box_to_world(k, i) * half_extents_m(i) * scale);
  }
  /* Not in the reference's class: collision queries for n oriented boxes moved along straight segments (host_motions[n][15]: the box as for
   * collidesOriented, then the displacement d xyz in sub-units; the attitude does not change) -- the min class over the voxels the moving box
   * touches and the exact parameter at which it first touches a blocking one -- se_hip_collide_oriented_motions_host, definitions in
   * se_hip.h.  host_out.status is required; a null t_first or t_exact means "not wanted".  stop_at is SE_HIP_COLLISION_OCCUPIED or
   * SE_HIP_COLLISION_UNSEEN.  The answers are those of se::geometry::oriented_motion_status (include/se/oriented_motion.hpp) on the
   * getMap() snapshot. */
  bool collidesOrientedMoving(const int32_t* host_motions, size_t n, const se_hip_collide_test& test, int32_t stop_at, se_hip_oriented_motion_out& host_out) {
    return ok(se_hip_collide_oriented_motions_host(h_, host_motions, (int64_t)n, &test, stop_at, &host_out));
  }
  /* The fifteen int32 of one such motion from a metric one: the box as orientedBox rounds it, then displacement_m (metres) rounded to the
   * nearest sub-unit like the centre (se::geometry::oriented_motion_round of include/se/oriented_motion.hpp does the same on plain arrays). */
  void orientedMotion(const Eigen::Matrix4f& box_to_world, const Eigen::Vector3f& half_extents_m, const Eigen::Vector3f& displacement_m, int32_t out[15]) const {
    const double scale = (double)SE_HIP_ORIENTED_SUB * volume_resolution_.x() / volume_dimension_.x();
    orientedBox(box_to_world, half_extents_m, out);
    for (int k = 0; k < 3; ++k) out[12 + k] = (int32_t)std::nearbyint(displacement_m(k) * scale);
  }
  /* Not in the reference's class: exact segment traces for n segments (host_segments[n][6]: a xyz, b xyz in sub-units of
   * 1 / SE_HIP_ORIENTED_SUB voxel) -- the min class on the way to the first blocking voxel, its entry parameter, the voxel, and the unseen /
   * empty voxels before it -- se_hip_trace_segments_host, definitions in se_hip.h.  host_out.status is required; a null pointer for another
   * array means "not wanted".  stop_at is SE_HIP_COLLISION_OCCUPIED or SE_HIP_COLLISION_UNSEEN.  The answers are those of
   * se::geometry::trace_walk (include/se/segment_trace.hpp) on the getMap() snapshot. */
  bool traceSegments(const int32_t* host_segments, size_t n, const se_hip_collide_test& test, int32_t stop_at, se_hip_trace_out& host_out) {
    return ok(se_hip_trace_segments_host(h_, host_segments, (int64_t)n, &test, stop_at, &host_out));
  }
  /* The six int32 of one such segment from metric endpoints: each coordinate x * 16 * size / dim is rounded to the nearest ODD sub-unit,
   * 2 rint((x - 1) / 2) + 1, so that an endpoint never lies on a voxel boundary and an axis-parallel segment never in a grid plane (where it
   * would touch nothing).  The trace is exact for the rounded segment; an endpoint moves by at most sqrt(3) / 16 voxel.  Values beyond int32
   * are clamped to it (such a segment is invalid anyway). */
  void segmentOf(const Eigen::Vector3f& a_m, const Eigen::Vector3f& b_m, int32_t out[6]) const {
    const double scale = (double)SE_HIP_ORIENTED_SUB * volume_resolution_.x() / volume_dimension_.x();
    for (int k = 0; k < 6; ++k) {
      const double x = (double)(k < 3 ? a_m(k) : b_m(k - 3)) * scale;
      const double odd = 2.0 * std::nearbyint((x - 1.0) / 2.0) + 1.0;
      out[k] = (int32_t)std::min(std::max(odd, -2147483647.0), 2147483647.0);
    }
  }
  /* Not in the reference's class (an addition of this mirror): se::functor::axis_aligned_map(map, f, min, max) for a list of n boxes with
   * f = "assign x and / or y where the current value has one of these classes", applied to the device map in list order without save / load --
   * se_hip_edit_boxes_host, definitions in se_hip.h.  The map afterwards is what se::apply_edits (include/se/axis_aligned.hpp) makes of the
   * getMap() snapshot taken before.  test may be null when every edit has only == 7; counts[4] (optional): voxel applications, node-value
   * applications, blocks touched, invalid edits. */
  bool editMap(const se_hip_edit* host_edits, size_t n, const se_hip_collide_test* test, int32_t mode, int64_t* counts = nullptr) {
    return ok(se_hip_edit_boxes_host(h_, host_edits, (int64_t)n, test, mode, counts));
  }
  /* Not in the reference's class (an addition of this mirror): Octree::allocate over the keys of every octant of a level that n voxel boxes touch,
   * on the device map without save / load -- se_hip_allocate_boxes_host, definitions in se_hip.h.  The map afterwards is what se::allocate_boxes
   * (include/se/allocate_region.hpp) makes of the getMap() snapshot taken before.  counts[4] (optional): blocks created, nodes created, requested
   * (box, octant) pairs, invalid boxes; new_keys (optional, capacity_words words): [count, key ...] of the octants created on request. */
  bool allocateRegion(const se_hip_alloc_box* host_boxes, size_t n, int64_t* counts = nullptr, uint64_t* new_keys = nullptr, int64_t capacity_words = 0) {
    return ok(se_hip_allocate_boxes_host(h_, host_boxes, (int64_t)n, counts, new_keys, capacity_words));
  }
  /* Not in the reference's class (an addition of this mirror): a rolling volume -- the map content translated by shift_voxels (multiples of 8,
   * the block side) on the device without save / load: content at voxel c is at c + s afterwards, what leaves the cube is forgotten, the vacated
   * side is unseen -- se_hip_shift_map, definitions in se_hip.h.  The map afterwards is what se::shift_map (include/se/shift_map.hpp) makes of the
   * getMap() snapshot taken before.  counts[4] (optional): blocks kept, blocks dropped, nodes kept, nodes dropped.  The camera moves with the
   * content: on success float(s[k]) * (volume_dimension / volume_resolution) is added to the translation of pose_ and to init_pose_, so
   * getPosition() is continuous across a shift up to the rounding of that addition (three float roundings) and setPose() keeps taking poses relative to the start.  raycast_pose_ and the vertex / normal
   * images stay in the old frame of reference: tracking() fails until raycasting() has run. */
  bool shiftMap(const Eigen::Vector3i& shift_voxels, int64_t* counts = nullptr) {
    const int32_t s[3] = {shift_voxels.x(), shift_voxels.y(), shift_voxels.z()};
    if (!ok(se_hip_shift_map(h_, s, counts))) return false;
    for (int k = 0; k < 3; ++k) {
      const float d = float(s[k]) * (volume_dimension_(k) / volume_resolution_(k));
      pose_(k, 3) += d;
      init_pose_(k) += d;
    }
    return true;
  }
  /* Not in the reference's class (an addition of this mirror): octants that lie wholly inside a box handed back on the device -- se_hip_release_boxes,
   * definitions in se_hip.h: SE_HIP_RELEASE_ALL forgets the region, SE_HIP_RELEASE_UNSEEN drops only what holds nothing but initValue().  The map
   * afterwards is what se::release_map (include/se/release_map.hpp) makes of the getMap() snapshot taken before.  counts[5] (optional): blocks
   * kept, released, nodes kept, released, released blocks that held an observed voxel; touched[6] (optional): lo and hi of the voxel box of the
   * released blocks.  The poses and the vertex / normal images stay as they are (tracking goes on).  A block that holds nothing but is still in
   * view and in the allocation band comes back with the next integrate(). */
  bool releaseMap(const std::vector<se_hip_release_box>& boxes, int64_t* counts = nullptr, int32_t* touched = nullptr) {
    return ok(se_hip_release_boxes(h_, boxes.empty() ? nullptr : boxes.data(), (int64_t)boxes.size(), counts, touched));
  }
  /* Not in the reference's class (an addition of this mirror): the content of another pipeline's map (same device, field type and voxel size; any
   * volume size) folded into this one on the device, source content at voxel c meeting this map's at c + shift_voxels (multiples of 8) --
   * se_hip_merge_map, definitions in se_hip.h.  The map afterwards is what se::merge_map (include/se/merge_map.hpp) makes of the two getMap()
   * snapshots taken before.  rule: SE_HIP_MERGE_FUSE / _REPLACE / _FILL and the SDF weight cap (default: FUSE, 100).  counts[12] (optional):
   * blocks combined, created, clipped, nodes combined, created, skipped, lo[3] and hi[3] of the voxel box of the blocks touched.  `other` is only
   * read; the poses and the vertex / normal images of both pipelines stay as they are (tracking goes on). */
  bool mergeMap(DenseSLAMSystem& other, const Eigen::Vector3i& shift_voxels = Eigen::Vector3i(0, 0, 0),
                const se_hip_merge_rule& rule = se_hip_merge_rule{SE_HIP_MERGE_FUSE, 100.f}, int64_t* counts = nullptr) {
    const int32_t s[3] = {shift_voxels.x(), shift_voxels.y(), shift_voxels.z()};
    return ok(se_hip_merge_map(h_, other.h_, s, &rule, counts));
  }
  /* Not in the reference's class (an addition of this mirror): the pull transform of se_hip_merge_map_rigid (src_from_dst, row-major 3 x 4, in
   * voxels) from the metric pose of the source map's frame in the destination's, x_dst = T_dst_src x_src, at voxel size dim / size: inverted and
   * scaled in double, rounded once.  False if the rotation part has no inverse. */
  static bool rigidPull(const Eigen::Matrix4f& T_dst_src, float dim, int size, float pull[12]) {
    double R[3][3], adj[3][3];
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) R[r][c] = (double)T_dst_src(r, c);
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j)
        adj[j][i] = R[(i + 1) % 3][(j + 1) % 3] * R[(i + 2) % 3][(j + 2) % 3] - R[(i + 1) % 3][(j + 2) % 3] * R[(i + 2) % 3][(j + 1) % 3];
    const double det = (R[0][0] * adj[0][0] + R[0][1] * adj[1][0]) + R[0][2] * adj[2][0];
    if (!(det != 0.0)) return false;
    const double scale = (double)size / (double)dim;
    for (int r = 0; r < 3; ++r) {
      double t = 0.0;
      for (int c = 0; c < 3; ++c) { pull[4 * r + c] = (float)(adj[r][c] / det); t += adj[r][c] / det * (double)T_dst_src(c, 3); }
      pull[4 * r + 3] = (float)(-t * scale);
    }
    return true;
  }
  /* Not in the reference's class (an addition of this mirror): the content of another pipeline's map (same device, field type and voxel size)
   * resampled into this one's lattice under a rigid transform and combined by `rule` -- se_hip_merge_map_rigid, definitions in se_hip.h.
   * T_dst_src is the metric pose of the other map's frame in this map's.  The map afterwards is what se::merge_map_rigid
   * (include/se/merge_rigid.hpp) makes of the two getMap() snapshots taken before, with the pull transform of rigidPull.  counts[10] (optional):
   * blocks that existed and received a sample, blocks created, voxels with a sample, of those observed before, lo[3] and hi[3] of the voxel box
   * of the blocks that received samples.  `other` is only read; poses and images of both pipelines stay as they are. */
  bool mergeMapRigid(DenseSLAMSystem& other, const Eigen::Matrix4f& T_dst_src,
                     const se_hip_merge_rule& rule = se_hip_merge_rule{SE_HIP_MERGE_FUSE, 100.f}, int64_t* counts = nullptr) {
    float pull[12];
    if (!rigidPull(T_dst_src, volume_dimension_(0), (int)volume_resolution_(0), pull)) return false;
    return ok(se_hip_merge_map_rigid(h_, other.h_, pull, &rule, counts));
  }
  /* Not in the reference's class (an addition of this mirror): the per-pixel body of raycastKernel for n rays of the caller's
   * (host_rays[n][8]: origin xyz, direction xyz, near, far in metres) answered on the device map without getMap() --
   * se_hip_cast_rays_host, definitions in se_hip.h.  host_out.hit[n][4], .normal[n][3], .status[n]; a null pointer: not wanted. */
  bool castRays(const float* host_rays, size_t n, float mu, se_hip_ray_out& host_out) {
    return ok(se_hip_cast_rays_host(h_, host_rays, (int64_t)n, mu, &host_out));
  }
  /* Not in the reference's class (an addition of this mirror): the triangles dump_mesh() would write, for the allocated blocks a region and up to
   * 64 views select, grouped per block in host memory -- se_hip_mesh_blocks_host, definitions in se_hip.h.  False (SE_HIP_E_CAPACITY) when
   * host_out is too small: host_out.header[0] and [1] then give the sizes needed. */
  bool meshBlocks(const se_hip_mesh_select& select, se_hip_mesh_out& host_out) {
    return ok(se_hip_mesh_blocks_host(h_, &select, &host_out));
  }
  /* vertex_ / normal_ of the last raycasting(): width*height packed xyz */
  bool getVertexNormal(std::vector<float>& vertex, std::vector<float>& normal) {
    const size_t n = (size_t)computation_size_.x() * computation_size_.y() * 3;
    vertex.resize(n); normal.resize(n);
    return ok(se_hip_download_vertex_normal(h_, vertex.data(), normal.data()));
  }

  bool getTracked() { return tracked_; }
  bool getIntegrated() { return integrated_; }
  Eigen::Vector3f getPosition() {
    return Eigen::Vector3f(pose_(0, 3) - init_pose_.x(), pose_(1, 3) - init_pose_.y(), pose_(2, 3) - init_pose_.z());
  }
  Eigen::Vector3f getInitPos() { return init_pose_; }
  Eigen::Matrix4f getPose() { return pose_; }
  /* DenseSLAMSystem.h:353-356: the translation is relative to the initial position */
  void setPose(const Eigen::Matrix4f pose) {
    pose_ = pose;
    pose_(0, 3) += init_pose_.x(); pose_(1, 3) += init_pose_.y(); pose_(2, 3) += init_pose_.z();
  }
  Eigen::Vector3f getModelDimensions() { return volume_dimension_; }
  Eigen::Vector3i getModelResolution() { return volume_resolution_; }
  Eigen::Vector2i getComputationResolution() { return computation_size_; }
  se_hip_pipeline* handle() { return h_; }
  /* every live pipeline of the process (what the argument-less synchroniseDevices() waits for) */
  static std::vector<se_hip_pipeline*>& live() { static std::vector<se_hip_pipeline*> l; return l; }

 private:
  static bool is_sdf();
  static Eigen::Matrix4f toMatrix4f(const Eigen::Vector3f& t) {  /* se_core/include/se/utils/math_utils.h:86-93 */
    Eigen::Matrix4f m = Eigen::Matrix4f::Identity();
    m(0, 3) = t.x(); m(1, 3) = t.y(); m(2, 3) = t.z();
    return m;
  }
  bool ok(int status) {
    if (status < 0) { std::cerr << "DenseSLAMSystem: " << se_hip_last_error() << std::endl; return false; }
    return true;
  }
  se_hip_pipeline* h_ = nullptr;
  Eigen::Vector2i computation_size_;
  Eigen::Vector3i volume_resolution_;
  Eigen::Vector3f volume_dimension_;
  Eigen::Vector3f init_pose_;
  Eigen::Matrix4f pose_, raycast_pose_;
  Eigen::Matrix4f* viewPose_ = &pose_;
  float mu_ = 0.1f;
  std::vector<int32_t> iterations_;
  bool tracked_ = false, integrated_ = false;
};

namespace se_hip_detail {
template <typename T> struct is_sdf_tag { static const bool value = false; };
template <> struct is_sdf_tag<SDF> { static const bool value = true; };
}  // namespace se_hip_detail
inline bool DenseSLAMSystem::is_sdf() { return se_hip_detail::is_sdf_tag<FieldType>::value; }

/* void synchroniseDevices(): declared and never defined in the reference (DenseSLAMSystem.h:418).  Its body here: wait for
 * everything every live DenseSLAMSystem of this process has enqueued on its device. */
inline void synchroniseDevices() { for (se_hip_pipeline* h : DenseSLAMSystem::live()) se_hip_sync(h); }
inline void synchroniseDevices(DenseSLAMSystem& s) { se_hip_sync(s.handle()); }

#endif /* SE_HIP_DENSESLAMSYSTEM_H */
